"""CPU: ubd_plan_stem (ubdvss_amd/csrc/stem_plan.h), the one place that chooses the form of the fp32 stem, built for the host.

stem_plan.h is plain C++, so a small program with its own main compiles it with the host compiler and prints the plan of every case
it reads.  The test compares it with the four rules restated in Python, with strips = n * ceil((H / 4) / 4) and
big = forced or strips >= 2 * num_cus:
  * strip form    <=>  inference and big and setting == 2 and fml
  * cold form     <=>  inference and not strip and not job and fml and (setting == 3 or (setting == 2 and not forced))
  * L1 + stem23   <=>  neither of the above, and inference and big and setting != 0
  * three kernels      otherwise
over the full product of the inputs below, and pins by name the cases that are easy to get wrong.
"""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include "stem_plan.h"
// stdin: one case per line (setting forced fml num_cus n H inference job); stdout: form, strip count, job-without-strips per case
int main()
{
    static_assert(UBD_STEM_SEPARATE == 0 && UBD_STEM_FUSED23 == 1 && UBD_STEM_FUSED123 == 2 && UBD_STEM_COLD123 == 3, "values of UBD_STEM");
    int setting, forced, fml, num_cus, n, H, inference, job;
    while (scanf("%d %d %d %d %d %d %d %d", &setting, &forced, &fml, &num_cus, &n, &H, &inference, &job) == 8) {
        const ubd_stem_plan p = ubd_plan_stem(setting, forced != 0, fml != 0, num_cus, n, H, inference != 0, job != 0);
        const char *form = p.form == UBD_STEM_FORM_SEPARATE ? "separate" : p.form == UBD_STEM_FORM_L1_STEM23 ? "l1_stem23" :
                           p.form == UBD_STEM_FORM_STRIPS ? "strips" : p.form == UBD_STEM_FORM_COLD ? "cold" : "?";
        printf("%s %ld %d\n", form, p.strips, p.job_without_strips ? 1 : 0);
    }
    return 0;
}
"""

SETTINGS = {"unfused": 0, "fused": 1, "fused123": 2, "cold123": 3}


def rules(setting, forced, fml, num_cus, n, H, inference, job):
    """the restatement: (form, strips, job given but the plan is not the strip form)"""
    strips = n * -(-(H // 4) // 4)
    big = bool(forced) or strips >= 2 * num_cus
    strip = bool(inference and big and setting == 2 and fml)
    cold = bool(inference and not strip and not job and fml and (setting == 3 or (setting == 2 and not forced)))
    if strip:
        form = "strips"
    elif cold:
        form = "cold"
    elif inference and big and setting != 0:
        form = "l1_stem23"
    else:
        form = "separate"
    return form, strips, int(bool(job) and form != "strips")


@pytest.fixture(scope="module")
def host_plan(tmp_path_factory):
    """runs the host build of stem_plan.h on a list of cases; returns one (form, strips, job_without_strips) per case"""
    work = tmp_path_factory.mktemp("stem_plan")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "a host C++ compiler is needed to build stem_plan.h for the CPU"
    (work / "plan.cpp").write_text(PROGRAM)
    subprocess.check_call([compiler, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ubdvss_amd", "csrc"),
                           "-o", str(work / "plan"), str(work / "plan.cpp")])

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
        out = subprocess.run([str(work / "plan")], input=text, stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout.split("\n")
        got = [(f, int(s), int(j)) for f, s, j in (line.split() for line in out if line)]
        assert len(got) == len(cases)
        return got
    return run


def test_plan_equals_the_four_rules_on_the_full_product(host_plan):
    cases = list(itertools.product(range(4), (0, 1), (0, 1), (1, 2, 3, 256, 304), (1, 2, 7, 32, 64, 683),
                                   (4, 8, 12, 16, 20, 512, 516, 1024), (0, 1), (0, 1)))
    assert len(cases) == 4 * 2 * 2 * 5 * 6 * 8 * 2 * 2
    got = host_plan(cases)
    wrong = [(c, g, rules(*c)) for c, g in zip(cases, got) if g != rules(*c)]
    assert not wrong, f"{len(wrong)} of {len(cases)} cases differ; first (case, header, rules): {wrong[:3]}"
    assert {g[0] for g in got} == {"separate", "l1_stem23", "strips", "cold"}


# (name, setting, forced, fml, num_cus, n, H, inference, job) -> (form, job given but the plan is not the strip form)
NAMED = [
    ("one 512 x 512 image, default, 256 CUs: 32 strips < 512", "fused123", 0, 1, 256, 1, 512, 1, 0, "cold", 0),
    ("32 x 512 x 512, default, 256 CUs: 1024 strips", "fused123", 0, 1, 256, 32, 512, 1, 0, "strips", 0),
    ("8 x 512 x 512, default, 256 CUs: 256 strips < 512", "fused123", 0, 1, 256, 8, 512, 1, 0, "cold", 0),
    ("16 x 512 x 512, default, 256 CUs: 512 strips, the threshold itself", "fused123", 0, 1, 256, 16, 512, 1, 0, "strips", 0),
    ("UBD_STEM=fused123 without fml padding", "fused123", 1, 0, 256, 1, 512, 1, 0, "l1_stem23", 0),
    ("UBD_STEM=cold123 with a job", "cold123", 1, 1, 256, 32, 512, 1, 1, "l1_stem23", 1),
    ("default, small launch, with a job: no cold form either", "fused123", 0, 1, 256, 1, 512, 1, 1, "separate", 1),
    ("default, big launch, with a job", "fused123", 0, 1, 256, 32, 512, 1, 1, "strips", 0),
    ("default without fml padding", "unfused", 0, 0, 256, 32, 512, 1, 0, "separate", 0),
    ("UBD_STEM=fused, small launch: forced", "fused", 1, 1, 256, 1, 64, 1, 0, "l1_stem23", 0),
]


@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_named_case(host_plan, case):
    _, setting, forced, fml, num_cus, n, H, inference, job, form, job_without = case
    args = (SETTINGS[setting], forced, fml, num_cus, n, H, inference, job)
    want = (form, n * ((H // 4 + 3) // 4), job_without)
    assert rules(*args) == want, "the restatement itself"
    assert host_plan([args]) == [want]


def test_training_runs_three_kernels_for_every_setting(host_plan):
    cases = [(s, forced, fml, cus, n, 512, 0, 0) for s in range(4) for forced in (0, 1) for fml in (0, 1) for cus in (2, 256) for n in (1, 64)]
    assert {g[0] for g in host_plan(cases)} == {"separate"}
