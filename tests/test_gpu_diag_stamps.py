"""GPU: the stamped diagnostic library (ubdvss_amd/csrc/stamps.h, build.sh diag) on the smallest shapes that reach every stamped
kernel.  The product library runs here; the diagnostic library runs in ONE fresh child process (a process loads one build), which checks
bit-equality with and without stamps, the stamps' order, the capacity bound and closeness to the product: tests/diag_stamp_cases.py."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diag_stamp_cases as dc  # noqa: E402

# a clean run of the child measured 2.2 s on an MI355X; 10 x that is 22 s, and the limit is never less than 60 s
CHILD_TIMEOUT_S = 60


@pytest.mark.gpu
def test_stamped_kernels_in_one_child_process(tmp_path):
    build = subprocess.run(["bash", os.path.join(ROOT, "ubdvss_amd", "csrc", "build.sh"), "diag"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-4000:]
    product = {}
    for name in dc.CASES:
        for k, v in dc.outputs(name).items():
            product[f"{name}/{k}"] = v
    npz = str(tmp_path / "product.npz")
    np.savez(npz, **product)
    t0 = time.time()
    child = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "diag_stamp_cases.py"), npz], capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    print(child.stdout)
    print(f"child process: {time.time() - t0:.1f} s")
    assert child.returncode == 0, child.stdout[-4000:] + child.stderr[-4000:]
    assert "DIAG_STAMPS_CHILD OK" in child.stdout
