// Handle lifecycle and error reporting of libubd_hip.so.
#include <stdarg.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include "common.h"

static thread_local char g_err[512] = "";

void ubd_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *ubd_last_error(void) { return g_err; }
extern "C" int ubd_abi_version(void) { return UBD_ABI_VERSION; }
#ifndef UBD_BUILD_ID
#define UBD_BUILD_ID "unknown"
#endif
// host staging helper (include/ubd.h): n bytes in `threads` contiguous pieces, one std::thread each (the caller's thread takes the first piece)
extern "C" int ubd_host_memcpy_mt(void *dst, const void *src, size_t n, int threads)
{
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    if (n < ((size_t)1 << 20)) threads = 1;
    const size_t piece = ((n + threads - 1) / threads + 4095) & ~(size_t)4095;
    std::thread th[16];
    int started = 0;
    size_t done_to = n < piece ? n : piece;              // [0, done_to) is the caller's piece; pieces whose thread could not be started are copied here too
    for (int t = 1; t < threads; ++t) {
        const size_t a = (size_t)t * piece;
        if (a >= n) break;
        const size_t len = n - a < piece ? n - a : piece;
        try {
            th[started] = std::thread([=] { memcpy((char *)dst + a, (const char *)src + a, len); });
            ++started;
        } catch (...) {                                  // no more threads to be had (resource limits): the rest in this thread
            memcpy((char *)dst + a, (const char *)src + a, n - a);
            break;
        }
    }
    memcpy(dst, src, done_to);
    for (int t = 0; t < started; ++t) th[t].join();
    return 0;
}
extern "C" const char *ubd_build_id(void) { return UBD_BUILD_ID; }   // sha256 over the kernel sources at build time (build.sh); bench.py compares it with the committed profiles' fingerprint

#ifdef UBD_STAMPS   // diagnostic build only (stamps.h): one stamp buffer per kernel family
// selectors: dilconv16s (d), dil_wgrad16 (d): the dilation; sepb16, sep_bwd (cin, stride): the template variant; the other families have none (0, 0)
static struct { const char *kernel; ubd_stamp_buf buf; int sel0, sel1; } g_stamps[] = {
    {"stem23"}, {"stem123"}, {"wino"}, {"wino6"}, {"sep123_16"}, {"dilconv16s"}, {"sepb16"}, {"sep_bwd"}, {"dil_wgrad16"}, {"postprocess"}, {"loss"},
};
extern "C" int ubd_debug_set_stamps(const char *kernel, void *buf, size_t capacity_words, int sel0, int sel1)
{
    for (auto &e : g_stamps)
        if (kernel && strcmp(kernel, e.kernel) == 0) {
            e.buf = {(unsigned long long *)buf, buf ? capacity_words : 0};
            e.sel0 = sel0; e.sel1 = sel1;
            return 0;
        }
    UBD_REQUIRE(false, "ubd_debug_set_stamps: no kernel family named %s", kernel ? kernel : "(null)");
}
ubd_stamp_buf ubd_stamps_for(const char *kernel, int sel0, int sel1)
{
    for (const auto &e : g_stamps)
        if (strcmp(kernel, e.kernel) == 0) return e.sel0 == sel0 && e.sel1 == sel1 ? e.buf : ubd_stamp_buf{nullptr, 0};
    return {nullptr, 0};
}
#endif

// The UBD_* environment switches, read once, when ubd_create builds the handle: NAME=value stores `set` in the int field at `field`; any
// other value is ignored.  What each field selects is written at the field (common.h).
static const char ANY[] = "", NUMBER[] = "#";      // in place of a value: set to anything / a positive integer, which is stored itself
struct env_switch { const char *name; size_t field; const char *value; int set; };
#define SW(name, field, value, set) {name, offsetof(ubd_handle, field), value, set}
static const env_switch ENV_SWITCHES[] = {
    SW("UBD_DILCONV", use_wino, "direct", 0), SW("UBD_DILCONV", wino_x6, "direct", 0), SW("UBD_DILCONV", wino_x6, "wino32", 0),
    SW("UBD_DILCONV", wino6_split3, "split3", 1),
    SW("UBD_WINO6_SPLIT", wino6_cvt_split, "cvt", 1),
    SW("UBD_WINO6_LAYOUT", wino6_natural, "natural", 1),
    SW("UBD_STEM", fuse_stem, "fused", UBD_STEM_FUSED23), SW("UBD_STEM", fuse_force, "fused", 1),
    SW("UBD_STEM", fuse_stem, "fused123", UBD_STEM_FUSED123), SW("UBD_STEM", fuse_force, "fused123", 1),
    SW("UBD_STEM", fuse_stem, "unfused", UBD_STEM_SEPARATE),
    SW("UBD_STEM123_SCHED", stem123_serial, "serial", 1),
    SW("UBD_TEST_NUM_CUS", num_cus, NUMBER, 0),
    SW("UBD_DILBWD", split_dilbwd, "split", 1), SW("UBD_DILBWD", no_pair_dilbwd, "pair8", 1),
    SW("UBD_SEPBWD", split_sepbwd32, "split", 1),
    SW("UBD_STEM16", split_stem16, "split", 1), SW("UBD_STEM16", split_stem16, "fused12", 2),
    SW("UBD_PP_GLOBAL", pp_global, ANY, 1), SW("UBD_PP_SPLIT", pp_split, ANY, 1), SW("UBD_PP_POISON", pp_poison, ANY, 1),
    SW("UBD_PP_SERIAL_TAIL", pp_serial_tail, ANY, 1), SW("UBD_PP_THREADS_512", pp_threads_512, ANY, 1),
    SW("UBD_HEADBWD", split_headbwd, "split", 1),
    SW("UBD_SEPB16_X", sepb_x_regs, "regs", 1),
    SW("UBD_REDUCE", chain_reduce, "batched", 0),
    SW("UBD_LOSS", loss_chain, "chain", 1),
    SW("UBD_DILCONV16", direct_dil16, "direct", 1),
};
#undef SW

extern "C" int ubd_create(const ubd_config *cfg, ubd_handle **out)
{
    UBD_REQUIRE(cfg && out, "ubd_create: null argument");
    UBD_REQUIRE(cfg->c_in == 1 || cfg->c_in == 3, "ubd_create: c_in must be 1 (grey) or 3, got %d", cfg->c_in);
    UBD_REQUIRE(cfg->n_classes >= 0 && cfg->n_classes <= UBD_MAX_CLASSES, "ubd_create: n_classes %d out of range [0,%d]", cfg->n_classes, UBD_MAX_CLASSES);
    UBD_REQUIRE(cfg->dtype == UBD_F32 || cfg->dtype == UBD_BF16 || cfg->dtype == UBD_F16, "ubd_create: bad dtype %d", cfg->dtype);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    UBD_REQUIRE(e == hipSuccess && ndev > 0, "ubd_create: no HIP device visible (%s); this library has no CPU fallback", hipGetErrorString(e));
    int dev = 0;
    UBD_CHECK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    UBD_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    UBD_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, "ubd_create: device arch %s is not gfx950; this library is built for MI355X only", prop.gcnArchName);

    ubd_handle *h = (ubd_handle *)calloc(1, sizeof(ubd_handle));
    UBD_REQUIRE(h, "ubd_create: out of host memory");
    h->cfg = *cfg;
    h->k_out = 1 + cfg->n_classes;
    h->num_cus = prop.multiProcessorCount;
    h->use_wino = h->wino_x6 = h->chain_reduce = 1;             // the defaults that are not 0
    h->fuse_stem = cfg->fml_compatible != 0 ? UBD_STEM_FUSED123 : UBD_STEM_SEPARATE;
    h->stem_cold_tail = -1;
    for (const env_switch &sw : ENV_SWITCHES) {
        const char *e = getenv(sw.name);
        if (!e) continue;
        int *field = (int *)((char *)h + sw.field);
        if (sw.value == NUMBER) { if (atoi(e) > 0) *field = atoi(e); }
        else if (sw.value == ANY || strcmp(e, sw.value) == 0) *field = sw.set;
    }
    { const char *s = getenv("UBD_STEM_COLD_TAIL"); if (s && *s >= '0' && *s <= '9') h->stem_cold_tail = atoi(s); }      // 0 is a value: not a table row
    { const char *s = getenv("UBD_STEM"); if (s && strcmp(s, "cold123") == 0 && cfg->fml_compatible != 0) { h->fuse_stem = UBD_STEM_COLD123; h->fuse_force = 1; } }      // fml padding only: not a table row
    // Keras model.get_weights() order
    size_t off = 0;
    int cin = cfg->c_in;
    for (int s = 0; s < 3; ++s) {
        h->off_sep_dw[s] = off; off += (size_t)9 * cin;
        h->off_sep_pw[s] = off; off += (size_t)cin * UBD_C;
        h->off_sep_b[s] = off;  off += UBD_C;
        cin = UBD_C;
    }
    for (int k = 0; k < UBD_NUM_DIL; ++k) {
        h->off_dil_k[k] = off; off += (size_t)9 * UBD_C * UBD_C;
        h->off_dil_b[k] = off; off += UBD_C;
    }
    h->off_head_k = off; off += (size_t)UBD_C * h->k_out;
    h->off_head_b = off; off += h->k_out;
    h->n_params = off;
    *out = h;
    return 0;
}

extern "C" void ubd_destroy(ubd_handle *h)
{
    if (h && h->comm) ubd_comm_destroy(h);
    free(h);
}

extern "C" size_t ubd_param_count(const ubd_handle *h) { return h ? h->n_params : 0; }
extern "C" int ubd_num_cus(const ubd_handle *h) { return h ? h->num_cus : 0; }
