"""Inputs on which floating-point arithmetic is exact, for tests that hold the kernels to BIT equality (not collected by pytest).

Images, kernels and biases are small integers times powers of two.  Every product is then exact, and when every partial sum of a
stage fits the 24 bits of an fp32 significand the stage's result is the same in ANY order of summation -- also on a matrix unit that
aligns its addends to the largest one before adding.  A 16-bit storage rounding is then a round-to-nearest-even of an exactly known
value, so the device has to return ``oracle.net_numpy.forward(..., act_dtype=...)`` bit for bit.  ``certificate`` measures the
condition (sum of |terms| over the terms' quantum, per stage); tests/test_exact_inputs_host.py asserts it (< 2^22) for every case
the GPU tests run, so the case tables below are certified rather than believed.

Case families (16-bit forward; the map side is a quarter of the image side):
  chain  all ten layers non-trivial (CHAIN): L1 dense ternary, L2 / L3 ternary at density 0.25 with pointwise kernels times 2^-2,
         L4..L9 ternary, alternately at density 0.08 times 2^-1 and at density 0.03, ternary head, biases in -2..2 times the layer's
         weight quantum;
  dense  layer k = 0..5 of the dilated ones dense (-2..2 at density 0.8), the other five centre-tap identities; the head either the
         24 x 24 identity (23 classes: the logits ARE L9's stored channels) or a dense integer detection head;
  small  as dense, with a sparse stem and a sparse layer k so that all of layer k's outputs stay below 2^8 quanta: every one is
         representable in bf16 as it is, so no storage rounding can absorb a one-unit error;
  stem   the six dilated layers identities and the identity head: the logits are L3's stored output; L2 / L3 at density 0.75.
fp32 layer cases (LAYER32_*): integer activations of both signs, dense kernels -2..2 times a power of two, integer biases, through
the Winograd forms and the direct form of one dilated layer; ``winograd_certificate`` states the transform-domain condition.

No case was dropped: every (case, type) of the tables is certified (DROPPED below stays empty and the host test checks that)."""
import collections
import functools

import numpy as np

from oracle import net_numpy as onet

DTYPES16 = ("bfloat16", "float16")
DIL = onet.DILATIONS
C = onet.N_FILTERS
MARGIN_LOG2 = 22            # sum |terms| / quantum stays below 2^22: two bits under the 24 of an fp32 significand
SMALL_LOG2 = {"bfloat16": 8, "float16": 11}     # significand bits of the storage types: below 2^that many quanta nothing is rounded
N_LAYERS = 10               # L1..L9 and the head: the length of a per-layer setting


def _per_layer(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * N_LAYERS


def exact_weights(seed, c_in=3, n_classes=0, density=1.0, scale=0, wmax=1, bmax=2):
    """The Keras-order weight list of ``oracle.net_numpy.weight_shapes`` with every kernel entry a non-zero integer in [-wmax, wmax]
    kept with probability ``density`` (else 0), times 2^scale; every bias an integer in [-bmax, bmax] times the quantum of the sums it
    is added to when the layer's inputs are integers (the product of the layer's kernel quanta).  ``density``, ``scale`` (exponents),
    ``wmax``, ``bmax``: one value or one per layer (L1..L9, head).  A separable layer's scale is carried by its POINTWISE kernel; its
    depthwise kernel stays integer.  float32 arrays (every value is exact in bf16 and fp16 too)."""
    density, scale, wmax, bmax = (_per_layer(v) for v in (density, scale, wmax, bmax))
    rng = np.random.default_rng(seed)
    out = []
    for name, shape in onet.weight_shapes(c_in, n_classes):
        li = N_LAYERS - 1 if name.startswith("head") else int(name[1]) - 1
        if name.endswith(".b"):
            w = rng.integers(-bmax[li], bmax[li] + 1, shape).astype(np.float64) * 2.0 ** scale[li]
        else:
            mag = rng.integers(1, wmax[li] + 1, shape) * rng.choice([-1, 1], shape)
            w = np.where(rng.random(shape) < density[li], mag, 0).astype(np.float64)
            if not name.endswith(".dw"):
                w = w * 2.0 ** scale[li]
        out.append(w.astype(np.float32))
    return out


def passthrough(weights, layers, identity_head=False):
    """A copy of ``weights`` in which the dilated layers ``layers`` (0..5) are centre-tap identities with zero bias: on the
    non-negative stored activations they return their input bit for bit.  ``identity_head``: the head becomes the 24 x 24 identity
    with zero bias (the list must be one of n_classes = 23)."""
    w = [np.array(a, copy=True) for a in weights]
    for k in layers:
        w[9 + 2 * k][:] = 0
        w[9 + 2 * k][1, 1] = np.eye(C, dtype=np.float32)
        w[10 + 2 * k][:] = 0
    if identity_head:
        assert w[-2].shape == (1, 1, C, C), "the identity head needs n_classes = 23"
        w[-2][0, 0] = np.eye(C, dtype=np.float32)
        w[-1][:] = 0
    return w


def exact_images(seed, n, h, w, c_in, top):
    """Integers in [0, top): (uint8, float32) arrays of shape (n, h, w, c_in)."""
    x = np.random.default_rng(seed).integers(0, top, (n, h, w, c_in), dtype=np.uint8)
    return x, x.astype(np.float32)


def quantum_log2(*arrays):
    """log2 of the largest power of two that divides every value of the arrays (None when all are zero)."""
    best = None
    for a in arrays:
        a = np.asarray(a, np.float64).ravel()
        a = a[a != 0]
        if a.size:
            m, e = np.frexp(a)
            i = np.abs(m * 2.0 ** 53).astype(np.int64)
            low = (np.log2((i & -i).astype(np.float64)) + e - 53).min()
            best = low if best is None else min(best, low)
    return None if best is None else int(best)


Stage = collections.namedtuple("Stage", "name log2_ratio max_stored min_stored quantum_log2")


def _stage(name, abs_sums, q_in, q_w, q_b, stored):
    """abs_sums: sum of |terms| (|bias| included) per output; q_*: quantum exponents of the inputs, the kernel, the bias (None: all zero)"""
    q = None if q_in is None or q_w is None else q_in + q_w
    if q_b is not None:
        q = q_b if q is None else min(q, q_b)
    top = float(np.max(abs_sums)) if np.size(abs_sums) else 0.0
    ratio = float("-inf") if top == 0 else float(np.log2(top)) - q
    nz = np.abs(stored[stored != 0]) if stored is not None else np.zeros(0)
    return Stage(name, ratio, float(np.abs(stored).max()) if stored is not None and stored.size else 0.0,
                 float(nz.min()) if nz.size else 0.0, q)


def certificate(x, weights, fml, act_dtype):
    """Per arithmetic stage of the 16-bit forward pass (each depthwise sum, each pointwise product, each dilated layer, the head), over
    all outputs: log2 of the largest (sum of |terms| including |bias|) / quantum, where the quantum of the terms is the largest power
    of two dividing every input value times that of the kernel, or the bias's if that is smaller; and the largest / smallest non-zero
    |value| the stage stores.  The sums of absolute values come from the oracle's own separable_conv / dilated_conv on absolute
    values in fp64; the inputs of each stage are the oracle's stored activations.  -> list of Stage."""
    f8 = np.float64
    w = [np.asarray(a, f8) for a in weights]
    x = np.asarray(x, f8)
    out = []
    eye = lambda c: np.eye(c, dtype=f8).reshape(1, 1, c, c)
    i = 0
    for li, stride in zip((1, 2, 3), (2, 1, 2)):
        dw, pw, b = onet.round_to(w[i], act_dtype), onet.round_to(w[i + 1], act_dtype), w[i + 2]
        c = x.shape[3]
        zero = np.zeros(c)
        dsum = onet.round_to(onet.separable_conv(x, dw, eye(c), zero, stride, fml, relu=False), act_dtype)     # the stored depthwise output
        dabs = onet.separable_conv(np.abs(x), np.abs(dw), eye(c), zero, stride, fml, relu=False)
        out.append(_stage(f"l{li}.dw", dabs, quantum_log2(x), quantum_log2(dw), None, dsum))
        y = onet.round_to(onet.separable_conv(x, dw, pw, b, stride, fml, act_dtype=act_dtype), act_dtype)
        pabs = np.abs(dsum) @ np.abs(pw[0, 0]) + np.abs(b)
        out.append(_stage(f"l{li}.pw", pabs, quantum_log2(dsum), quantum_log2(pw), quantum_log2(b), y))
        x = y
        i += 3
    for li, d in zip(range(4, 10), DIL):
        k, b = onet.round_to(w[i], act_dtype), w[i + 1]
        y = onet.round_to(onet.dilated_conv(x, k, b, d), act_dtype)
        kabs = onet.dilated_conv(np.abs(x), np.abs(k), np.abs(b), d, relu=False)
        out.append(_stage(f"l{li}", kabs, quantum_log2(x), quantum_log2(k), quantum_log2(b), y))
        x = y
        i += 2
    habs = np.abs(x) @ np.abs(w[i][0, 0]) + np.abs(w[i + 1])
    out.append(_stage("head", habs, quantum_log2(x), quantum_log2(w[i]), quantum_log2(w[i + 1]), x @ w[i][0, 0] + w[i + 1]))
    return out


# ---------------------------------------------------------------------------------------------------------------- 16-bit cases

Case = collections.namedtuple("Case", "name kind n mh mw c_in n_classes fml seed layer")

# map sizes (n, rows, columns) and what they reach: 1 x 9: dilation 1 staged in LDS (the staged kernel needs ceil(W4 / d) > 8); 1 x 132:
# dilation 16 staged on a one-row map; 5 x 129: a ragged last staged tile at dilation 16; 33 x 144: exactly 9 sub-grid columns and 3
# sub-grid rows at dilation 16; 17 x 37: tiles cut by both borders, direct kernel for d >= 8; 18 x 26: the 72 x 104 image
CHAIN_MAPS = ((1, 1, 1), (1, 2, 3), (1, 1, 9), (1, 1, 132), (1, 5, 129), (1, 33, 144), (2, 17, 37), (3, 18, 26))
# settings of the chain family: with every dilated layer at 2^-1 the quantum gets one bit finer per layer while fp16 keeps 11 bits of
# every value, and sum |terms| / quantum passes 2^24 on the 33 x 144 map; alternating 2^-1 layers with sparser integer ones keeps the
# magnitudes level (largest stored value about 1400) and the worst ratio at 2^19.8
CHAIN = dict(top=16, density=(1.0, 0.25, 0.25) + (0.08, 0.03) * 3 + (1.0,), scale=(0, -2, -2) + (-1, 0) * 3 + (0,), wmax=1, bmax=2)
# the stem family alone (identity layers behind it) has room for a denser L2 / L3: over its cases every stem weight is non-zero once
STEM = dict(CHAIN, density=(1.0, 0.75, 0.75) + CHAIN["density"][3:])
SMALL = dict(top=2, density=(1.0, 0.15, 0.15) + (0.04,) * 6 + (1.0,), scale=0, wmax=1, bmax=1)
STEM_MAPS = ((1, 1, 1), (1, 2, 3), (2, 17, 37), (3, 18, 26))
# (UBD_STEM16 or None for the one-kernel stem, input form, c_in, fml_compatible): nine rows that cover every PAIR of values of the four
# factors (3 stems x 3 input forms in full; c_in and the padding rule balanced across them).  Forms: "u8" = uint8 with
# PreprocessingType.NONE, "f32" = float32 at a 16-byte-aligned address (LDS-DMA input path), "f32_off4" = float32 through a view one
# element past such an address (register-staged input path)
STEM_RUNS = ((None, "u8", 3, True), (None, "f32", 1, False), (None, "f32_off4", 3, False),
             ("split", "u8", 1, False), ("split", "f32", 3, True), ("split", "f32_off4", 1, True),
             ("fused12", "u8", 3, False), ("fused12", "f32", 1, True), ("fused12", "f32_off4", 3, True))
ONE_CU_CASE = "chain_3x18x26_cls0"          # also run with UBD_TEST_NUM_CUS=1: persistent blocks walk several tiles
TRAIN_CASES = ("chain_3x18x26_cls0", "chain_2x17x37_cls0")


def dense_maps(k):
    """1 x 1, 2 x 3, the two smallest maps that put layer k's dilation into the LDS-staged kernel, and 17 x 37"""
    d = DIL[k]
    return ((1, 1, 1), (1, 2, 3), (1, 1, 8 * d + 1), (1, 2, 8 * d + 2), (2, 17, 37))


def _cases():
    out, seed = [], 1000
    for n, mh, mw in CHAIN_MAPS:
        for ncls in (0, 2):
            seed += 1
            out.append(Case(f"chain_{n}x{mh}x{mw}_cls{ncls}", "chain", n, mh, mw, 3, ncls, True, seed, None))
    for k in range(6):
        for n, mh, mw in dense_maps(k):
            for ncls in (23, 0):
                seed += 1
                out.append(Case(f"dense{k}_{n}x{mh}x{mw}_{'ident' if ncls else 'head'}", "dense", n, mh, mw, 3, ncls, True, seed, k))
        seed += 1
        out.append(Case(f"small{k}_2x17x37_ident", "small", 2, 17, 37, 3, 23, True, seed, k))
    for n, mh, mw in STEM_MAPS:
        for c_in in (1, 3):
            for fml in (True, False):
                seed += 1
                out.append(Case(f"stem_{n}x{mh}x{mw}_c{c_in}_{'fml' if fml else 'same'}", "stem", n, mh, mw, c_in, 23, fml, seed, None))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
DROPPED = {dt: [] for dt in DTYPES16}          # (case name, reason) of inputs the host test could not certify: none


def cases(kind, **match):
    return [c for c in CASES if c.kind == kind and all(getattr(c, f) == v for f, v in match.items())]


@functools.lru_cache(maxsize=None)
def build(case):
    """-> (uint8 images, the same as float32, weights) of a case; deterministic in the case's seed.  Treat as read-only."""
    others = [k for k in range(6) if k != case.layer]
    if case.kind in ("chain", "stem"):
        s = dict(CHAIN if case.kind == "chain" else STEM)
        w = exact_weights(case.seed, case.c_in, case.n_classes, s["density"], s["scale"], s["wmax"], s["bmax"])
        if case.kind == "stem":
            w = passthrough(w, range(6), identity_head=True)
    elif case.kind == "dense":
        s = dict(CHAIN)
        wmax = [1] * N_LAYERS
        density = list(s["density"])
        scale = list(s["scale"])
        wmax[3 + case.layer], density[3 + case.layer], scale[3 + case.layer] = 2, 0.8, 0
        wmax[9] = 3                                                                   # the dense integer head: -3..3
        w = passthrough(exact_weights(case.seed, case.c_in, case.n_classes, density, scale, wmax, s["bmax"]), others, case.n_classes == 23)
    else:
        s = dict(SMALL)
        w = passthrough(exact_weights(case.seed, case.c_in, case.n_classes, s["density"], s["scale"], s["wmax"], s["bmax"]), others, True)
    x8, xf = exact_images(case.seed + 500000, case.n, 4 * case.mh, 4 * case.mw, case.c_in, s["top"])
    for a in (x8, xf, *w):
        a.setflags(write=False)
    return x8, xf, tuple(w)


@functools.lru_cache(maxsize=None)
def reference(case, dtype, eval_dtype="float64"):
    """-> (logits, the nine stored activations) of the oracle with ``dtype`` storage, evaluated in ``eval_dtype``.  Read-only."""
    _, xf, w = build(case)
    lg, acts = onet.forward(xf, list(w), case.fml, dtype=np.dtype(eval_dtype).type, return_all=True, act_dtype=dtype)
    for a in (lg, *acts):
        a.setflags(write=False)
    return lg, tuple(acts)


@functools.lru_cache(maxsize=None)
def certify(case, dtype):
    _, xf, w = build(case)
    return tuple(certificate(xf, w, case.fml, dtype))


def first_difference(got, want):
    """message naming the first differing (image, row, column, channel) of two equally shaped arrays and both values"""
    if got.shape != want.shape:
        return f"shapes differ: {got.shape} against {want.shape}"
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if not len(bad):
        return "equal"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {got.size} differ, first at (image, row, column, channel) = {i}: got {got[i]!r}, want {want[i]!r}"


# ---------------------------------------------------------------------------------------------------- oracle mutations (host only)

def weights_one_quantum_off(case, layer):
    """the case's weights with one entry (tap (2, 0), input channel 5, output channel 7) of dilated layer ``layer`` raised by one quantum"""
    w = [np.array(a, copy=True) for a in build(case)[2]]
    w[9 + 2 * layer][2, 0, 5, 7] += np.float32(2.0 ** quantum_log2(w[9 + 2 * layer]))
    return w


def mutated_logits(case, dtype, layer, kind):
    """The oracle's logits with ONE deliberate fault in dilated layer ``layer`` (0..5) -- what a kernel fault of that kind would return:
    "weight": one kernel entry raised by one quantum; "halo": the left halo one column too narrow, so that the left taps of ONE output
    column (d - 1, whose left neighbour at distance d is the last padding column) read map column 0 instead of zero; "bias": the bias left out; "truncate": the storage rounding of the layer's output replaced by truncation."""
    w = [np.asarray(a, np.float64) for a in (weights_one_quantum_off(case, layer) if kind == "weight" else build(case)[2])]
    ki, d = 9 + 2 * layer, DIL[layer]
    _, acts = reference(case, dtype)
    x = acts[2 + layer]                                     # the layer's input: a3 for layer 0
    k, b = onet.round_to(w[ki], dtype), (np.zeros(C) if kind == "bias" else w[ki + 1])
    if kind == "halo":
        assert d - 1 < x.shape[2]
        edge = np.pad(x[:, :, 0, :], ((0, 0), (d, d), (0, 0)))                   # map column 0 with the layer's row padding
        acc = onet.dilated_conv(x, k, b, d, relu=False)
        for ky in range(3):                                                      # the three left taps of output column d - 1 read column 0
            acc[:, :, d - 1, :] += edge[:, ky * d:ky * d + x.shape[1], :] @ k[ky, 0]
        y = np.maximum(acc, 0)
    else:
        y = onet.dilated_conv(x, k, b, d)
    x = truncate_to(y, dtype) if kind == "truncate" else onet.round_to(y, dtype)
    for j in range(layer + 1, 6):
        x = onet.round_to(onet.dilated_conv(x, onet.round_to(w[9 + 2 * j], dtype), w[10 + 2 * j], DIL[j]), dtype)
    return x @ w[-2][0, 0] + w[-1]


def truncate_to(a, act_dtype):
    """a (non-negative, exactly representable in fp32) cut to the 16-bit type's significand instead of rounded"""
    bits = SMALL_LOG2[act_dtype]
    m, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(np.floor(m * 2.0 ** bits), e - bits)


def mutated_stem_logits(case, dtype, kind):
    """As mutated_logits for the stem: "dw": one depthwise tap of L2 raised by one; "pw": one pointwise weight of L3 raised by one quantum;
    "padding": the other stride-2 padding rule."""
    _, xf, w = build(case)
    w = [np.array(a, np.float64) for a in w]
    if kind == "dw":
        w[3][0, 2, 11, 0] += 1.0
    elif kind == "pw":
        w[7][0, 0, 3, 9] += 2.0 ** quantum_log2(w[7])
    return onet.forward(xf, w, case.fml if kind != "padding" else not case.fml, act_dtype=dtype)


# ------------------------------------------------------------------------------------------------------- fp32 dilated-layer cases

LAYER32_SHAPES = ((1, 1, 1), (1, 2, 3), (3, 37, 91), (2, 72, 100))
LAYER32_TOP = 64                                 # activations: integers in [-64, 64)
LAYER32_WSCALE = (0, -3, 2, -1, 0, -6)           # per layer: kernels are integers in -2..2 (density 0.8) times 2^that
LAYER32_SCALES = (0, -30, 30)                    # the inputs and biases times 2^that must give the outputs times 2^that, bit for bit


@functools.lru_cache(maxsize=None)
def layer32_weights():
    """(3, 3, 24, 24) kernels and (24,) biases of the six layers: integers in -2..2 at density 0.8 times 2^LAYER32_WSCALE[k]; biases
    integers in -8..8 times the same quantum (the inputs are integers).  float64, read-only."""
    rng = np.random.default_rng(32)
    out = []
    for k in range(6):
        kern = np.where(rng.random((3, 3, C, C)) < 0.8, rng.integers(1, 3, (3, 3, C, C)) * rng.choice([-1, 1], (3, 3, C, C)), 0)
        q = 2.0 ** LAYER32_WSCALE[k]
        out += [kern * q, rng.integers(-8, 9, C) * q]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def layer32_input(shape):
    x = np.random.default_rng(sum(shape)).integers(-LAYER32_TOP, LAYER32_TOP, (*shape, C)).astype(np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def layer32_reference(shape, k):
    """relu(conv + bias) of layer k in fp64 (exact: the sums stay far below 2^53 quanta)"""
    w = layer32_weights()
    y = onet.dilated_conv(layer32_input(shape), w[2 * k], w[2 * k + 1], DIL[k])
    y.setflags(write=False)
    return y


_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])
_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)

Wino = collections.namedtuple("Wino", "log2_products log2_output bits_sample bits_weight")


def winograd_certificate(x, kern, bias):
    """The exactness condition of one fp32 dilated layer computed as F(2x2, 3x3) (G holds 0, +-1, +-1/2; B and A hold 0, +-1), in units of
    1/4 times the quantum of the inputs times that of the kernel:
      log2_products  per transform point and output channel, the sum over the 24 input channels of |V| |U|, with U = G g G^T and V = B^T d B
                     bounded through |d| <= max |x| (every entry of V adds four samples with signs);
      log2_output    the output transform's sum of |terms| (each output adds nine of the products' sums) plus |bias|;
      bits_sample    significant bits of the largest transformed sample (two fp16 pieces hold 22);
      bits_weight    significant bits of the largest transformed kernel entry (one fp16 piece holds 11: the product of the second pieces,
                     which the two-piece form drops, is then zero).
    The same bounds cover the direct form, whose terms are a subset."""
    qx, qw = quantum_log2(x), quantum_log2(kern)
    unit = 2.0 ** (qx + qw - 2)
    u = np.einsum("ai,ijco,bj->abco", _G, np.asarray(kern, np.float64), _G)              # (4, 4, c_in, c_out)
    vmax = np.abs(_BT).sum(1).max() ** 2 * float(np.abs(x).max())                        # 4 max|x|
    prod = (vmax * np.abs(u).sum(2)).max()                                               # over points and output channels
    a_terms = np.abs(_AT).sum(1).max() ** 2                                              # 9
    outp = a_terms * prod + float(np.abs(bias).max())
    assert quantum_log2(bias) is None or quantum_log2(bias) >= qx + qw - 2
    bits = lambda v: int(np.ceil(np.log2(v + 1)))
    return Wino(float(np.log2(prod / unit)), float(np.log2(outp / unit)), bits(vmax / 2.0 ** qx), bits(np.abs(u).max() / 2.0 ** (qw - 2)))
