// Which form the fp32 stem (L1 -> L2 -> L3) takes for one launch: the ONE place that decides it.  Plain C++ (no HIP, no ubd_handle), so
// a host compiler builds it alone (tests/test_stem_plan_host.py).
#pragma once

// ubd_handle::fuse_stem, from UBD_STEM (api.hip).  Default: UBD_STEM_FUSED123 with the fml padding (the variant that inherits the 33rd L2
// column from the tile to its left: 0.405 vs 0.417 ms per forward pass at 32 x 512 x 512), else UBD_STEM_SEPARATE -- with TF 'same'
// padding the fused kernel only ties the separate kernels.  ubd_handle::fuse_force: UBD_STEM named the variant, so it
// is taken at any launch size.
enum {
    UBD_STEM_SEPARATE = 0,    // UBD_STEM=unfused: three kernels
    UBD_STEM_FUSED23 = 1,     // UBD_STEM=fused: L1, then L2 -> L3 fused with L2's output in LDS (stem23.h)
    UBD_STEM_FUSED123 = 2,    // UBD_STEM=fused123: L1 -> L2 -> L3 in one kernel (stem123.h); by itself it walks strips in big launches and cold tiles in small ones
    UBD_STEM_COLD123 = 3,     // UBD_STEM=cold123: that kernel with one cold-started tile per work unit at any size (fml padding only; tests)
};

enum ubd_stem_form {
    UBD_STEM_FORM_SEPARATE,   // three sepconv_kernel launches
    UBD_STEM_FORM_L1_STEM23,  // sepconv_kernel for L1 + stem23_kernel
    UBD_STEM_FORM_STRIPS,     // stem123_kernel, every block walks whole strips of tiles; the only form that can carry a postprocess job
    UBD_STEM_FORM_COLD,       // stem123_kernel<COLD>, one tile per work unit
};

#define UBD_STEM_STRIP_ROWS 4   // L3 rows of a strip of tiles (s23_cfg::TH3)

struct ubd_stem_plan {
    ubd_stem_form form;
    long strips;              // n * ceil(H4 / UBD_STEM_STRIP_ROWS): the work units of the strip form, the tile rows of the cold form
    bool job_without_strips;  // a postprocess job was given, but the plan is not the strip form: the caller must refuse
    int tail_rows;            // strip form with a job: the last tail_rows strips (in ticket order) are walked as cold tiles (stem123.h); else 0
};

// Default tail of a job pass: rows per block that runs a postprocess job first.  Such a block joins the strip queue a job (~90 us) late;
// at 32 x 512 x 512 the 1024 strips are then 4.57 rounds of the other 224 blocks and half of them run a fifth strip of ~28 us.  With 4 rows
// per job block in the tail the strips are 224 x 4 exactly, and the 128 tail rows go out as cold tiles of ~3.4 us (a ninth tile per row of
// eight).  Measured, not derived: 0 .. 96 rows gain nothing, 128 and 192 the same (profiles/r08_ab_cold_tail_sweep.txt).  Tuned at that ONE
// shape, where 4 is also the strips per block: at other batch sizes and heights the remaining strips are no whole number of rounds (batch
// 64: 1920 strips on 224 blocks = 8.57 rounds) and the tail is unmeasured there; UBD_STEM_COLD_TAIL sets it per process.
#define UBD_STEM_TAIL_ROWS_PER_JOB_BLOCK 4

// setting / forced / fml: the handle's fuse_stem, fuse_force, cfg.fml_compatible; job: a postprocess job rides along.
// The fused kernels give every CU whole strips of tiles: they need ~2 strips per CU to fill the chip (a single 512 x 512 image has 32
// for 256 CUs), so smaller launches take one cold tile per work unit -- or, where that form does not apply (no fml padding, a job, a
// forced variant), the three separate kernels.  Training always runs the separate kernels.
// W, job_maps, tail_override: image width, maps of the postprocess job, UBD_STEM_COLD_TAIL (< 0: unset) -- the inputs of tail_rows.  The
// tail is clipped so that the D strips every block owns without a ticket (stem123.h: one for rows of three or more tiles, else
// 4 - tiles) remain strips.
static inline ubd_stem_plan ubd_plan_stem(int setting, bool forced, bool fml, int num_cus, int n, int H, bool inference, bool job,
                                          int W = 0, int job_maps = 0, int tail_override = -1)
{
    ubd_stem_plan p;
    p.strips = (long)n * ((H / 4 + UBD_STEM_STRIP_ROWS - 1) / UBD_STEM_STRIP_ROWS);
    const bool big = forced || p.strips >= 2L * num_cus;
    if (inference && big && setting == UBD_STEM_FUSED123 && fml) p.form = UBD_STEM_FORM_STRIPS;
    else if (inference && !job && fml && (setting == UBD_STEM_COLD123 || (setting == UBD_STEM_FUSED123 && !forced))) p.form = UBD_STEM_FORM_COLD;
    else if (inference && big && setting != UBD_STEM_SEPARATE) p.form = UBD_STEM_FORM_L1_STEM23;
    else p.form = UBD_STEM_FORM_SEPARATE;
    p.job_without_strips = job && p.form != UBD_STEM_FORM_STRIPS;
    p.tail_rows = 0;
    if (p.form == UBD_STEM_FORM_STRIPS && job && job_maps > 0 && W > 0) {
        const long grid = p.strips < num_cus ? p.strips : num_cus;
        const int tiles_x = (W / 4 + 15) / 16, D = tiles_x >= 3 ? 1 : 4 - tiles_x;
        const long job_blocks = job_maps < grid ? job_maps : grid;
        const long want = tail_override >= 0 ? tail_override : (long)UBD_STEM_TAIL_ROWS_PER_JOB_BLOCK * job_blocks;
        const long room = p.strips - grid * D;
        p.tail_rows = (int)(want < room ? want : (room > 0 ? room : 0));
    }
    return p;
}
