"""GPU: the cold-tile tail of a job pass of the one-kernel stem (stem123.h, ubd_plan_stem's tail_rows).

With a postprocess job riding along, the last R strips of the pass (in ticket order) are handed out as single cold-started tiles from
a second ticket counter.  Every output is computed by the instructions of the strip walk on the same values, so the logits and every
output of the job are BIT-EQUAL to the pass with UBD_STEM_COLD_TAIL=0, for R = 1, R = half the rows and R >= all the rows that may be
cold (the plan clips R so that the strips a block owns without a ticket stay strips).  Two passes in a row on one workspace: the strip,
tile and check-out counters reset themselves.

At the default grid the small shapes below have no more strips than blocks own statically, so the plan clips their tail to 0 (that
clipping is then what runs); the 70 x 64 x 192 case has 280 strips for 256 blocks and a real tail of up to 24 rows there too.  That a tail
really ran is checked, not assumed: ubd_stem_tail_rows reports the rows of the launch's own plan, and every case on the 2-CU grid and
the 70-image case must report min(R, room) > 0 rows; the unset switch (the default) is one of the sides."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import net_numpy as onet
from ubdvss_amd import NetConfig, Model, PreprocessingType, synthetic

pytestmark = pytest.mark.gpu

N_CLS = 2
CAP = 64

# name -> (n, H, W, grey, uint8, maps of the job, grids)
CASES = {
    "3x64x64 one tile per row": (3, 64, 64, False, False, 3, ("2", None)),
    "2x72x132 ragged last tile row, second tile of one column": (2, 72, 132, False, False, 2, ("2", None)),
    "2x64x512 nine cold tiles per row": (2, 64, 512, False, False, 2, ("2", None)),
    "5x64x260 five maps on two blocks": (5, 64, 260, False, False, 5, ("2",)),
    "3x64x196 grey": (3, 64, 196, True, False, 3, ("2", None)),
    "3x64x196 uint8": (3, 64, 196, False, True, 3, ("2", None)),
    "70x64x192 more strips than the default grid owns": (70, 64, 192, False, False, 8, (None,)),
}


def _job_outputs(outs):
    """what the library specifies of a job's outputs: map, counts, and each list up to its count"""
    bmap, quads, classes, counts = (t.cpu().numpy() for t in outs)
    k = np.minimum(counts, CAP)
    return bmap, counts, [q[:c] for q, c in zip(quads, k)], [cl[:c] for cl, c in zip(classes, k)]


def _room(grid, n, hh, ww):
    """rows that may be cold: the strips beyond those every block owns without a ticket (restated from stem_plan.h)"""
    strips = n * ((hh // 4 + 3) // 4)
    blocks = min(strips, 256 if grid is None else int(grid))
    tiles = (ww // 4 + 15) // 16
    return max(strips - blocks * (1 if tiles >= 3 else 4 - tiles), 0)


def _passes(monkeypatch, tail, grid, cfg, w, xt, lg, want_rows=None):
    """two job passes in a row on one model (one workspace) under UBD_STEM_COLD_TAIL=tail (None: unset, the plan's default):
    [(logits, job outputs)] * 2.  want_rows: the tail the launch must really use (ubd_stem_tail_rows reports the launch's own plan)."""
    monkeypatch.setenv("UBD_STEM", "fused123")
    if tail is None: monkeypatch.delenv("UBD_STEM_COLD_TAIL", raising=False)
    else: monkeypatch.setenv("UBD_STEM_COLD_TAIL", str(tail))
    if grid is None: monkeypatch.delenv("UBD_TEST_NUM_CUS", raising=False)
    else: monkeypatch.setenv("UBD_TEST_NUM_CUS", grid)
    m = Model(cfg)
    m.set_weights(w)
    if grid is not None: assert m.num_cus == int(grid)
    n, hh, ww, _ = xt.shape
    tail_rows = m._lib.ubd_stem_tail_rows                                          # a diagnostic export: declared here, as tools/_diag.py declares its own
    tail_rows.restype, tail_rows.argtypes = ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4
    rows = int(tail_rows(m._h, n, hh, ww, lg.shape[0]))
    if want_rows is not None: assert rows == want_rows, (tail, grid, rows, want_rows)
    assert int(tail_rows(m._h, n, hh, ww, -1)) == 0, "no job, no tail"
    outs = m.alloc_postprocess_outputs(lg.shape[0], lg.shape[1], lg.shape[2], CAP)
    job = {"logits": lg, "logit_threshold": 0.0, "scale": 4, "min_area": 5, "cap": CAP, "outputs": outs}
    out = torch.empty((n, hh // 4, ww // 4, 1 + N_CLS), device="cuda")
    res = []
    for _ in range(2):
        out.fill_(float("nan"))                                                   # a tile nobody wrote shows
        for t in outs: t.fill_(-3)
        m.predict_on_device(xt, out=out, postprocess=job)
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), _job_outputs(outs)))
    return res


def _equal(a, b):
    (la, (ma, ca, qa, cla)), (lb, (mb, cb, qb, clb)) = a, b
    return (np.array_equal(la, lb) and np.array_equal(ma, mb) and np.array_equal(ca, cb)
            and all(np.array_equal(x, y) for x, y in zip(qa, qb)) and all(np.array_equal(x, y) for x, y in zip(cla, clb)))


@pytest.mark.parametrize("name", list(CASES))
def test_cold_tail_is_bit_equal_to_the_strip_walk(name, monkeypatch):
    n, hh, ww, grey, u8, maps, grids = CASES[name]
    cin = 1 if grey else 3
    cfg = NetConfig(class_names=["a", "b"], grey=grey, preprocessing=PreprocessingType.MOBILENET_LIKE if u8 else PreprocessingType.NONE)
    w = onet.init_weights(31, cin, N_CLS, bias_scale=0.2)
    xt = torch.from_numpy(synthetic.noise_images(5, n, hh, ww, cin, as_float=not u8)).cuda()
    lab = synthetic.rectangle_maps(17, maps, 48, 80, n_classes=N_CLS)            # the job's maps need not have the pass's shape
    lg = torch.from_numpy(synthetic.logits_from_maps(lab, N_CLS, seed=18)).cuda()
    rows = n * ((hh // 4 + 3) // 4)
    for grid in grids:
        room = _room(grid, n, hh, ww)
        if grid == "2" or n == 70: assert room > 0, "this case must have a real tail"
        ref = _passes(monkeypatch, 0, grid, cfg, w, xt, lg, want_rows=0)
        assert not np.isnan(ref[0][0]).any() and int(ref[0][1][1].max()) > 0, "the reference side itself: every logit written, objects found"
        assert _equal(ref[1], ref[0])
        for tail in (1, rows // 2, rows, 1 << 20, None):                             # None: the default, 4 rows per job block
            want = min(4 * min(maps, 256 if grid is None else int(grid)) if tail is None else tail, room)
            got = _passes(monkeypatch, tail, grid, cfg, w, xt, lg, want_rows=want)
            for k in range(2):
                assert _equal(got[k], ref[0]), (name, grid, tail, k, int((got[k][0] != ref[0][0]).sum()))
