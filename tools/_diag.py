"""What the tools that run the diagnostic library share (bash ubdvss_amd/csrc/build.sh diag -> tools/_ab/libubd_hip_diag.so: every
kernel of ubdvss_amd/csrc/stamps.h takes a stamp buffer): loading it in place of the product library, and one stamped call.

    import _diag                         # first: puts the repository root on sys.path
    lib = _diag.load()                   # before anything of ubdvss_amd creates a handle
    s = _diag.stamps(lib, "wino6", (8192, 8), lambda: run(layer))     # int64 numpy array of that shape, 0 = slot not written

Kernel families and their selectors (the table in api.hip): stem23, stem123, wino, wino6, sep123_16, postprocess, loss: none;
dilconv16s, dil_wgrad16: sel = (dilation,); sepb16, sep_bwd: sel = (cin, stride)."""
import ctypes, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)
from ubdvss_amd import _lib


def load(name=None):
    """Loads tools/_ab/<name> (default: $DIAG_LIB or libubd_hip_diag.so) as THE library of this process and declares the one setter."""
    _lib.LIB_PATH = os.path.join(ROOT, "tools", "_ab", name or os.environ.get("DIAG_LIB", "libubd_hip_diag.so"))
    lib = _lib.load()
    lib.ubd_debug_set_stamps.restype = ctypes.c_int
    lib.ubd_debug_set_stamps.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    return lib


def stamps(lib, kernel, shape, call, sel=(), reps=1, capacity=None, fill=0):
    """call() `reps` times with a buffer of `shape` 64-bit words (filled with `fill`) registered for `kernel`; the buffer as numpy.
    capacity: register fewer words than allocated (the kernels store below the registered capacity only)."""
    st = torch.full(shape, fill, dtype=torch.int64, device="cuda")
    sel = tuple(sel) + (0, 0)
    _lib.check(lib.ubd_debug_set_stamps(kernel.encode(), st.data_ptr(), st.numel() if capacity is None else capacity, sel[0], sel[1]), "ubd_debug_set_stamps")
    try:
        for _ in range(reps): call()
        torch.cuda.synchronize()
    finally:
        lib.ubd_debug_set_stamps(kernel.encode(), None, 0, 0, 0)
    return st.cpu().numpy()
