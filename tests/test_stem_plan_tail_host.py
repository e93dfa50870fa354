"""CPU: the tail rows of ubd_plan_stem (ubdvss_amd/csrc/stem_plan.h), built for the host as tests/test_stem_plan_host.py builds the form.

tail_rows is the number of strips at the end of a job pass that the one-kernel stem hands out as single cold-started tiles.  Restated:
  * 0 unless the plan is the strip form AND a job with at least one map rides along AND the width is known
  * else min(want, room) with
      grid  = min(strips, num_cus),  tiles = ceil((W / 4) / 16),  D = 1 if tiles >= 3 else 4 - tiles   (strips a block owns unasked)
      room  = max(strips - grid * D, 0)                                                                  (those strips stay strips)
      want  = UBD_STEM_COLD_TAIL if it is set (>= 0), else UBD_STEM_TAIL_ROWS_PER_JOB_BLOCK * min(job maps, grid)
The form, the strip count and job_without_strips do not depend on the three new arguments, and a call without them plans no tail."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include "stem_plan.h"
// stdin: one case per line (setting forced fml num_cus n H inference job W job_maps override); stdout per case: form, tail rows with the
// three tail arguments, tail rows without them, whether form / strips / job_without_strips are the same in both calls; first line: the constant
int main()
{
    printf("%d\n", (int)UBD_STEM_TAIL_ROWS_PER_JOB_BLOCK);
    int setting, forced, fml, num_cus, n, H, inference, job, W, maps, over;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d", &setting, &forced, &fml, &num_cus, &n, &H, &inference, &job, &W, &maps, &over) == 11) {
        const ubd_stem_plan p = ubd_plan_stem(setting, forced != 0, fml != 0, num_cus, n, H, inference != 0, job != 0, W, maps, over);
        const ubd_stem_plan q = ubd_plan_stem(setting, forced != 0, fml != 0, num_cus, n, H, inference != 0, job != 0);
        printf("%d %d %d %d\n", (int)p.form, p.tail_rows, q.tail_rows, p.form == q.form && p.strips == q.strips && p.job_without_strips == q.job_without_strips);
    }
    return 0;
}
"""

FORMS = {"separate": 0, "l1_stem23": 1, "strips": 2, "cold": 3}


@pytest.fixture(scope="module")
def host_plan(tmp_path_factory):
    work = tmp_path_factory.mktemp("stem_plan_tail")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "a host C++ compiler is needed to build stem_plan.h for the CPU"
    (work / "plan.cpp").write_text(PROGRAM)
    subprocess.check_call([compiler, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ubdvss_amd", "csrc"),
                           "-o", str(work / "plan"), str(work / "plan.cpp")])

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
        out = subprocess.run([str(work / "plan")], input=text, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout.split("\n")
        rows = [tuple(int(v) for v in line.split()) for line in out if line]
        assert len(rows) == len(cases) + 1
        return rows[0][0], rows[1:]
    return run


def rules(per_job_block, setting, forced, fml, num_cus, n, H, inference, job, W, maps, over):
    strips = n * -(-(H // 4) // 4)
    big = bool(forced) or strips >= 2 * num_cus
    if not (inference and big and setting == 2 and fml and job and maps > 0 and W > 0):
        return 0
    grid = min(strips, num_cus)
    tiles = -(-(W // 4) // 16)
    d = 1 if tiles >= 3 else 4 - tiles
    want = over if over >= 0 else per_job_block * min(maps, grid)
    return min(want, max(strips - grid * d, 0))


def test_tail_rows_equal_the_restatement_on_the_full_product(host_plan):
    cases = list(itertools.product(range(4), (0, 1), (0, 1), (2, 256), (1, 5, 32, 70), (64, 72, 512), (0, 1), (0, 1),
                                   (0, 64, 132, 260, 512), (0, 1, 5, 32, 300), (-1, 0, 1, 96, 1 << 20)))
    const, got = host_plan(cases)
    assert const >= 0
    wrong = [(c, g, rules(const, *c)) for c, g in zip(cases, got) if g[1] != rules(const, *c)]
    assert not wrong, f"{len(wrong)} of {len(cases)} cases differ; first (case, program, rules): {wrong[:3]}"
    assert all(g[2] == 0 and g[3] == 1 for g in got), "without the tail arguments: no tail, and the same form / strips / job_without_strips"
    assert all(g[1] == 0 for c, g in zip(cases, got) if g[0] != FORMS["strips"] or not c[7]), "only a job pass of the strip form has a tail"
    assert any(g[1] > 0 for g in got)


# (name, num_cus, n, H, W, job, maps, override) -> tail rows; setting fused123, fml, inference; forced where the launch is small
NAMED = [
    ("headline 32 x 512 x 512, 32 maps, R = 128: 1024 strips, 256 owned", 256, 32, 512, 512, 1, 32, 128, 128),
    ("headline, R = 0: the reference side", 256, 32, 512, 512, 1, 32, 0, 0),
    ("headline, huge R: clipped to 1024 - 256", 256, 32, 512, 512, 1, 32, 1 << 20, 768),
    ("headline without a job: the override does not apply", 256, 32, 512, 512, 0, 0, 128, 0),
    ("3 x 64 x 64 on 2 CUs: one tile per row, D = 3, 12 - 6 rows of room", 2, 3, 64, 64, 1, 3, 1 << 20, 6),
    ("2 x 72 x 132 on 2 CUs: five rows per image, three tiles per row, D = 1", 2, 2, 72, 132, 1, 2, 1 << 20, 8),
    ("2 x 64 x 512 on 2 CUs", 2, 2, 64, 512, 1, 2, 3, 3),
    ("2 x 64 x 512 at 256 CUs: 8 strips, all owned", 256, 2, 64, 512, 1, 2, 3, 0),
    ("3 x 64 x 64 at 256 CUs: fewer strips than owned slots", 256, 3, 64, 64, 1, 3, 1 << 20, 0),
    ("70 x 64 x 192 at 256 CUs: 280 strips, 24 rows of room", 256, 70, 64, 192, 1, 8, 1 << 20, 24),
]


@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_named_case(host_plan, case):
    _, num_cus, n, H, W, job, maps, over, want = case
    args = (2, 1, 1, num_cus, n, H, 1, job, W, maps, over)
    const, got = host_plan([args])
    assert rules(const, *args) == want, "the restatement itself"
    assert got[0][1] == want


def test_default_is_the_constant_times_the_job_blocks_and_is_clipped(host_plan):
    const, got = host_plan([(2, 0, 1, 256, 32, 512, 1, 1, 512, m, -1) for m in (1, 8, 32, 300)])
    assert [g[1] for g in got] == [min(const * min(m, 256), 768) for m in (1, 8, 32, 300)]
