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

fp32 forward cases (Case32, CASES32; nothing is rounded between the stages, so every setting is integer and sparser than its 16-bit
counterpart; tests/test_gpu_exact32.py):
  stem32   identity dilated layers and identity head: the logits are L3's output.  Six settings (STEM32_SETTINGS) on seven map sizes
           (STEM32_MAPS), grey and RGB, both stride-2 padding rules;
  chain32  all ten layers non-trivial (CHAIN32) on the CHAIN_MAPS sizes, 0 and 2 classes;
  head32   the dense stem, identity dilated layers and a dense integer head (-3..3) of 1, 3 and 32 output channels.
Piece liveness.  The fp32 stem computes L2's and L3's pointwise products as three-way bf16 split products (csrc/split3.h): of the nine
products (sample piece i) x (weight piece j) the six with i + j <= 4 are kept (KEPT).  A kept product that is zero everywhere could be
dropped or mis-slotted by a kernel without any test noticing, so the stem32 settings are chosen such that, for L2 and for L3 each on its
own, every kept product is non-zero for some (pixel, input channel, output channel) of some case -- and the three dropped products are
zero everywhere in every case, or the kernel would legitimately differ from the oracle.  ``split3`` restates the truncation split,
``split3_certificate`` measures the liveness, ``forward32_mutated`` leaves one product out of the oracle; the host test asserts all three.

No case was dropped: every (case, type) of the tables is certified (DROPPED and DROPPED32 below stay empty and the host test checks that)."""
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
    """act_dtype None: the fp32 forward pass, nothing is rounded between the stages.
    Per arithmetic stage of the 16-bit forward pass (each depthwise sum, each pointwise product, each dilated layer, the head), over
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


def winograd_certificate(x, kern, bias, per_channel=False):
    """The exactness condition of one fp32 dilated layer computed as F(2x2, 3x3) (G holds 0, +-1, +-1/2; B and A hold 0, +-1), in units of
    1/4 times the quantum of the inputs times that of the kernel:
      log2_products  per transform point and output channel, the sum over the 24 input channels of |V| |U|, with U = G g G^T and V = B^T d B
                     bounded through |d| <= max |x| (every entry of V adds four samples with signs);
      log2_output    the output transform's sum of |terms| (each output adds nine of the products' sums) plus |bias|;
      bits_sample    significant bits of the largest transformed sample (two fp16 pieces hold 22);
      bits_weight    significant bits of the largest transformed kernel entry (one fp16 piece holds 11: the product of the second pieces,
                     which the two-piece form drops, is then zero).
    The same bounds cover the direct form, whose terms are a subset.
    per_channel: the same sums bounded more closely -- |d| <= max |x| of the sample's own input channel, and each output adds the
    products' sums its own entries of A select (|A^T| x |A^T|) instead of nine times the largest; for a centre-tap identity kernel
    that is four products of at most max |x| of the channel."""
    qx, qw = quantum_log2(x), quantum_log2(kern)
    unit = 2.0 ** (qx + qw - 2)
    u = np.einsum("ai,ijco,bj->abco", _G, np.asarray(kern, np.float64), _G)              # (4, 4, c_in, c_out)
    vmax = np.abs(_BT).sum(1).max() ** 2 * float(np.abs(x).max())                        # 4 max|x|
    prod = (vmax * np.abs(u).sum(2)).max()                                               # over points and output channels
    a_terms = np.abs(_AT).sum(1).max() ** 2                                              # 9
    outp = a_terms * prod + float(np.abs(bias).max())
    if per_channel:
        vc = np.abs(_BT).sum(1).max() ** 2 * np.abs(x).reshape(-1, x.shape[-1]).max(0)   # (c_in,)
        prods = np.einsum("c,abco->abo", vc, np.abs(u))
        prod = prods.max()
        outp = (np.einsum("ia,jb,abo->ijo", np.abs(_AT), np.abs(_AT), prods) + np.abs(bias)).max()
    assert quantum_log2(bias) is None or quantum_log2(bias) >= qx + qw - 2
    bits = lambda v: int(np.ceil(np.log2(v + 1)))
    return Wino(float(np.log2(prod / unit)), float(np.log2(outp / unit)), bits(vmax / 2.0 ** qx), bits(np.abs(u).max() / 2.0 ** (qw - 2)))


# ------------------------------------------------------------------------------------------------ fp32 forward cases (no storage rounding)

KEPT = ((1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (3, 1))      # (sample piece, weight piece) products split3.h keeps: i + j <= 4
DROPPED_PRODUCTS = ((2, 3), (3, 2), (3, 3))


def split3(v):
    """The truncation split of ubdvss_amd/csrc/split3.h (split3_bits) restated: v (exactly representable in fp32) -> its three bf16
    pieces, float64 arrays of v's shape with v == p1 + p2 + p3: p1 = the high 16 bits of v's fp32 pattern, p2 = those of v - p1, p3 =
    those of v - p1 - p2 (every subtraction is exact in fp32)."""
    v = np.ascontiguousarray(v, np.float32)
    assert np.array_equal(v.astype(np.float64), np.asarray(v, np.float64))
    hi16 = lambda a: (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    p1 = hi16(v)
    r1 = v - p1
    p2 = hi16(r1)
    r2 = r1 - p2
    p3 = hi16(r2)
    assert np.array_equal(r2, p3), "three pieces hold all 24 bits"
    return tuple(p.astype(np.float64) for p in (p1, p2, p3))


def split3_certificate(samples, pw):
    """One pointwise stage computed as split products: samples (..., c) = the depthwise sums, pw (c, c_out).  -> 3 x 3 bool array, entry
    [i - 1][j - 1]: the product (sample piece i) x (weight piece j) is non-zero for some (pixel, input channel, output channel).  Asserts
    that the pieces re-add to the values exactly."""
    sp, wp = split3(samples), split3(pw)
    assert np.array_equal(sp[0] + sp[1] + sp[2], np.asarray(samples, np.float64))
    assert np.array_equal(wp[0] + wp[1] + wp[2], np.asarray(pw, np.float64))
    c = pw.shape[0]
    live = np.zeros((3, 3), bool)
    for i in range(3):
        s_nz = (sp[i].reshape(-1, c) != 0).any(0)                  # per input channel: some pixel has a non-zero piece i
        for j in range(3):
            live[i, j] = bool((s_nz & (wp[j] != 0).any(1)).any())
    return live


def split_pointwise(samples, pw, bias, leave_out=None, relu=True):
    """relu(samples @ pw + bias) as the sum of the six kept piece products (fp64: exact on certified inputs); leave_out: one (i, j) of
    KEPT that is dropped too -- what a schedule that loses that product would return."""
    sp, wp = split3(samples), split3(pw)
    y = np.zeros(samples.shape[:-1] + (pw.shape[1],))
    for i, j in KEPT:
        if (i, j) != leave_out:
            y = y + sp[i - 1] @ wp[j - 1]
    y = y + np.asarray(bias, np.float64)
    return np.maximum(y, 0) if relu else y


def depthwise_sums(x, dw, stride, fml):
    """the depthwise stage of a separable layer alone (fp64): what the pointwise product reads"""
    c = x.shape[3]
    return onet.separable_conv(np.asarray(x, np.float64), np.asarray(dw, np.float64), np.eye(c).reshape(1, 1, c, c), np.zeros(c), stride, fml, relu=False)


Case32 = collections.namedtuple("Case32", "name kind setting n mh mw c_in n_classes fml seed")

# Map sizes (n, rows, columns) of the fp32 stem cases and what they reach.  A stem tile is 16 L3 columns by 4 L3 rows (stem23.h: 16 lanes of a unit, TH3);
# cold-started tiles sit 15 columns apart (stem123.h: cold_kx); a strip is one tile row of one image (stem_plan.h).
#   1 x 1, 2 x 3   the smallest maps: every tile edge is an image edge
#   5 x 17         a second tile one column wide (its first L2 column is the carried / recomputed one) and a second tile row one row high
#   2 x 31         cold tiles at columns 0, 15 and 30, the last one column wide; two strip tiles
#   3 x 33         three strip tiles: the carried 33rd L2 column is handed on twice; cold tiles at 0, 15, 30
#   2 x 17 x 37    tiles cut by both borders, a ragged last tile row, two images
#   3 x 18 x 26    the 72 x 104 image, three images
STEM32_MAPS = ((1, 1, 1), (1, 2, 3), (1, 5, 17), (1, 2, 31), (1, 3, 33), (2, 17, 37), (3, 18, 26))

# Settings of the stem32 family.  ``base``: the arguments of exact_weights (ternary kernels at a density per layer, biases in -bmax..bmax
# times the layer's quantum); ``top``: images are integers in [0, top), a pair: for grey and for RGB images (a grey L1 adds one term where
# an RGB one adds three).  Two overrides per separable layer 0..2 (L1..L3) bound the number
# of terms of a sum exactly instead of by a density:
#   ``dw``: {layer: taps}: the depthwise kernel has exactly ``taps`` of its nine taps non-zero (+-1) per channel;
#   ``pw``: {layer: (lo, hi, terms)}: the pointwise kernel has exactly ``terms`` non-zero input channels per output channel (all of them
#           when the layer has fewer inputs), integers in [lo, hi) with random signs.
# A product of piece i of a sample and piece j of a weight is live when the sample spans more than 8 (i - 1) significant bits and the
# weight more than 8 (j - 1); a term must fit fp32 -- sample bits + weight bits + log2(terms) <= 22 -- so three pieces on one side go with
# one piece on the other, and (2, 2) with about nine bits on each side.  A3 must stay below 2^18 quanta: behind it an identity Winograd
# layer adds four transformed products of up to max |A3| each, in quarter quanta (winograd_certificate: output sums < 2^22).  So wide L2
# values are followed by an L3 of one tap and one term.  What each setting is for (certified per case by the host test):
#   dense   the 16-bit STEM setting: every stem weight non-zero in some case; one-piece values, (1, 1) only; fits uint8
#   wide_s  images below 8192 (grey) / 4096 (RGB), float32 only: samples of up to 18 bits against weights +-1: (1, 1), (2, 1), (3, 1) at L2 and at L3
#   wide_w2 L2's weights 17 bits wide against samples 0, +-1, +-2 (0 / 1 images, one tap and one term per kernel, biases -1..1): (1, 2),
#           (1, 3) at L2; twice the largest weight plus the biases stays below 2^18
#   wide_w3 the same at L3 (no bias at L1, so that L3's samples are 0, +-1, +-2)
#   mid2    nine-bit samples against nine-bit weights (256 .. 383) at L2, one term: (2, 2) there
#   mid3    the same at L3
_D32 = (0.08, 0.03) * 3 + (1.0,)          # densities of L4..L9 and the head before passthrough replaces them
STEM32_SETTINGS = {
    "dense": dict(top=16, base=dict(density=(1.0, 0.75, 0.75) + _D32, scale=(0, -2, -2) + (0,) * 7, wmax=1, bmax=2), dw={}, pw={}),
    "wide_s": dict(top=(8192, 4096), base=dict(density=(1.0, 0.25, 0.25) + _D32, scale=0, wmax=1, bmax=2), dw={2: 1}, pw={1: (1, 2, 2), 2: (1, 2, 1)}),
    "wide_w2": dict(top=2, base=dict(density=(1.0, 0.25, 0.25) + _D32, scale=0, wmax=1, bmax=1), dw={0: 1, 1: 1, 2: 1},
                    pw={0: (1, 2, 1), 1: (2 ** 16, 2 ** 17 - 2, 1), 2: (1, 2, 1)}),
    "wide_w3": dict(top=2, base=dict(density=(1.0, 0.25, 0.25) + _D32, scale=0, wmax=1, bmax=(0, 1, 1) + (0,) * 7), dw={0: 1, 1: 1, 2: 1},
                    pw={0: (1, 2, 1), 1: (1, 2, 1), 2: (2 ** 16, 2 ** 17 - 2, 1)}),
    "mid2": dict(top=(40, 16), base=dict(density=(1.0, 0.25, 0.25) + _D32, scale=0, wmax=1, bmax=2), dw={2: 1}, pw={1: (256, 384, 1), 2: (1, 2, 1)}),
    "mid3": dict(top=(28, 11), base=dict(density=(1.0, 0.25, 0.25) + _D32, scale=0, wmax=1, bmax=2), dw={}, pw={1: (1, 2, 3), 2: (256, 384, 1)}),
}
U8_SETTINGS = tuple(s for s, v in STEM32_SETTINGS.items() if np.max(v["top"]) <= 256)      # images that exist as uint8


def sparse_pointwise(rng, rows, lo, hi, terms):
    """(1, 1, rows, 24) pointwise kernel: per output channel exactly min(terms, rows) non-zero input channels, integers in [lo, hi)
    with random signs"""
    k = np.zeros((rows, C))
    terms = min(terms, rows)
    for o in range(C):
        ch = rng.choice(rows, terms, replace=False)
        k[ch, o] = rng.integers(lo, hi, terms) * rng.choice([-1, 1], terms)
    return k.reshape(1, 1, rows, C).astype(np.float32)


def sparse_depthwise(rng, channels, taps):
    """(3, 3, channels, 1) depthwise kernel with exactly ``taps`` non-zero taps (+-1) per channel"""
    k = np.zeros((9, channels))
    for c in range(channels):
        k[rng.choice(9, taps, replace=False), c] = rng.choice([-1, 1], taps)
    return k.reshape(3, 3, channels, 1).astype(np.float32)


def stem32_weights(seed, c_in, setting):
    """identity dilated layers and identity head behind a stem of the given STEM32_SETTINGS entry"""
    s = STEM32_SETTINGS[setting]
    w = exact_weights(seed, c_in, 23, **s["base"])
    rng = np.random.default_rng(seed + 77)
    for layer, taps in sorted(s["dw"].items()):
        w[3 * layer] = sparse_depthwise(rng, w[3 * layer].shape[2], taps)
    for layer, (lo, hi, terms) in sorted(s["pw"].items()):
        w[3 * layer + 1] = sparse_pointwise(rng, w[3 * layer + 1].shape[2], lo, hi, terms)
    return passthrough(w, range(6), identity_head=True)


# (UBD_STEM or None, input form, c_in, fml_compatible): fifteen rows, every (stem, input form) pair, that cover every PAIR of values of the
# four factors.  With 'same' padding the one-kernel forms do not apply: the handle then runs what it honours (unset, cold123, unfused: three
# sepconv_kernel launches; fused123, fused: sepconv_kernel + stem23_kernel) and that is what is checked.  Forms as in STEM_RUNS; "u8" runs
# the settings whose images exist as uint8 (U8_SETTINGS), the float32 forms all of them.
STEM32_RUNS = ((None, "u8", 1, False), (None, "f32", 3, True), (None, "f32_off4", 1, True),
               ("fused123", "u8", 3, True), ("fused123", "f32", 1, True), ("fused123", "f32_off4", 3, False),
               ("cold123", "u8", 1, True), ("cold123", "f32", 3, False), ("cold123", "f32_off4", 1, True),
               ("fused", "u8", 3, True), ("fused", "f32", 1, False), ("fused", "f32_off4", 3, False),
               ("unfused", "u8", 1, False), ("unfused", "f32", 3, True), ("unfused", "f32_off4", 3, True))
# settings of the chain32 family: see CHAIN; without storage rounding nothing is cut back between the layers, so the scaled layers of CHAIN
# (each makes the quantum finer while the magnitudes stay) are integer here and the dilated layers sparser: the worst stage stays below
# 2^22 quanta and every dilated layer's Winograd-domain sums below 2^22 quarter quanta on the 33 x 144 map too
CHAIN32 = dict(top=4, density=(1.0, 0.25, 0.25) + (0.04, 0.025) * 3 + (1.0,), scale=0, wmax=1, bmax=1)
HEAD32_CLASSES = (0, 2, 31)
HEAD32_MAPS = ((1, 1, 1), (1, 2, 3), (2, 17, 37))
ONE_CU_CASE32 = "chain32_3x18x26_cls0"
TRAIN_CASES32 = ("chain32_3x18x26_cls0", "chain32_2x17x37_cls0")
TAIL_CASE32 = "head32_2x17x37_cls2"                  # the job pass with a cold tail: 10 strips of three tiles on two blocks
TEETH_PW3_CASE32 = "stem32_wide_w3_2x17x37_c3_fml"   # (1, 3) live at L3
TEETH_DW2_CASE32 = "stem32_dense_2x17x37_c3_fml"


def _cases32():
    out, seed = [], 32000
    for setting in STEM32_SETTINGS:
        for n, mh, mw in STEM32_MAPS:
            for c_in in (1, 3):
                for fml in (True, False):
                    seed += 1
                    out.append(Case32(f"stem32_{setting}_{n}x{mh}x{mw}_c{c_in}_{'fml' if fml else 'same'}", "stem32", setting, n, mh, mw, c_in, 23, fml, seed))
    for n, mh, mw in CHAIN_MAPS:
        for ncls in (0, 2):
            seed += 1
            out.append(Case32(f"chain32_{n}x{mh}x{mw}_cls{ncls}", "chain32", None, n, mh, mw, 3, ncls, True, seed))
    for n, mh, mw in HEAD32_MAPS:
        for ncls in HEAD32_CLASSES:
            seed += 1
            out.append(Case32(f"head32_{n}x{mh}x{mw}_cls{ncls}", "head32", None, n, mh, mw, 3, ncls, True, seed))
    return out


CASES32 = _cases32()
BY_NAME32 = {c.name: c for c in CASES32}
DROPPED32 = []                                  # (case name, reason) of fp32 inputs the host test could not certify: none


def cases32(kind, **match):
    return [c for c in CASES32 if c.kind == kind and all(getattr(c, f) == v for f, v in match.items())]


@functools.lru_cache(maxsize=None)
def build32(case):
    """-> (uint8 images or None when they do not fit, the same as float32, weights) of an fp32 case.  Treat as read-only."""
    if case.kind == "stem32":
        top = STEM32_SETTINGS[case.setting]["top"]
        top = top[case.c_in // 2] if isinstance(top, tuple) else top
        w = stem32_weights(case.seed, case.c_in, case.setting)
    elif case.kind == "chain32":
        s = dict(CHAIN32)
        top = s.pop("top")
        w = exact_weights(case.seed, case.c_in, case.n_classes, **s)
    else:                                       # head32: the dense stem, identity dilated layers, a dense integer head in -3..3
        s = STEM32_SETTINGS["dense"]
        top = s["top"]
        base = dict(s["base"], wmax=(1,) * 9 + (3,))
        w = passthrough(exact_weights(case.seed, case.c_in, case.n_classes, **base), range(6))
    xf = np.random.default_rng(case.seed + 500000).integers(0, top, (case.n, 4 * case.mh, 4 * case.mw, case.c_in)).astype(np.float32)
    x8 = xf.astype(np.uint8) if top <= 256 else None
    for a in (x8, xf, *w):
        if a is not None:
            a.setflags(write=False)
    return x8, xf, tuple(w)


@functools.lru_cache(maxsize=None)
def reference32(case, eval_dtype="float64"):
    """-> (logits, the nine activations) of the oracle without storage rounding, evaluated in ``eval_dtype``.  Read-only."""
    _, xf, w = build32(case)
    lg, acts = onet.forward(xf, list(w), case.fml, dtype=np.dtype(eval_dtype).type, return_all=True)
    for a in (lg, *acts):
        a.setflags(write=False)
    return lg, tuple(acts)


@functools.lru_cache(maxsize=None)
def certify32(case):
    _, xf, w = build32(case)
    return tuple(certificate(xf, w, case.fml, None))


@functools.lru_cache(maxsize=None)
def split_liveness32(case):
    """-> (3 x 3 liveness of the piece products of L2's pointwise stage, the same of L3's) on the oracle's own depthwise sums"""
    _, _, w = build32(case)
    acts = reference32(case)[1]
    return (split3_certificate(depthwise_sums(acts[0], w[3], 1, case.fml), w[4][0, 0]),
            split3_certificate(depthwise_sums(acts[1], w[6], 2, case.fml), w[7][0, 0]))


def forward32_mutated(case, kind, arg=None, weights=None):
    """The oracle's fp32-path logits with ONE deliberate fault (host only; ``kind`` None: no fault, the oracle itself):
      ("drop", (layer 2 | 3, (i, j)))  the kept piece product (sample piece i, weight piece j) left out of that layer's pointwise sum;
      "dw"        tap (0, 2) of channel 11 of L2's depthwise kernel raised by one;
      "padding"   the other stride-2 padding rule;
      "bias3"     L3's bias left out;
      "head_bias" the head's bias left out.
    L2's and L3's pointwise stages are evaluated as the sum of the kept piece products (split_pointwise), the rest by the oracle.
    weights: in place of the case's own (the device-side teeth)."""
    _, xf, w = build32(case)
    w = [np.array(a, np.float64) for a in (w if weights is None else weights)]
    fml = case.fml if kind != "padding" else not case.fml
    if kind == "dw":
        w[3][0, 2, 11, 0] += 1.0
    if kind == "bias3":
        w[8][:] = 0
    if kind == "head_bias":
        w[-1][:] = 0
    drop = arg if kind == "drop" else (None, None)
    x = onet.separable_conv(np.asarray(xf, np.float64), w[0], w[1], w[2], 2, fml)
    x = split_pointwise(depthwise_sums(x, w[3], 1, fml), w[4][0, 0], w[5], drop[1] if drop[0] == 2 else None)
    x = split_pointwise(depthwise_sums(x, w[6], 2, fml), w[7][0, 0], w[8], drop[1] if drop[0] == 3 else None)
    for k, d in enumerate(DIL):
        x = onet.dilated_conv(x, w[9 + 2 * k], w[10 + 2 * k], d)
    return x @ w[-2][0, 0] + w[-1]


def pw3_third_piece_entry(case):
    """-> ((input channel, output channel), unit): an entry of the case's L3 pointwise kernel and the unit (the kernel's quantum) by which
    raising it changes its THIRD piece alone -- the first such entry for which the oracle's logits change"""
    k = build32(case)[2][7][0, 0]
    p = split3(k)
    unit = np.float32(2.0 ** quantum_log2(k))
    for ci, co in np.argwhere(p[1] != 0):
        q = split3(np.float32(k[ci, co] + unit).reshape(1))
        if q[0][0] == p[0][ci, co] and q[1][0] == p[1][ci, co] and q[2][0] != p[2][ci, co]:
            if not np.array_equal(forward32_mutated(case, None, weights=weights_pw3_raised(case, (int(ci), int(co)), float(unit))), reference32(case)[0]):
                return (int(ci), int(co)), float(unit)
    raise AssertionError("no such entry")


def weights_pw3_raised(case, entry, unit):
    w = [np.array(a, copy=True) for a in build32(case)[2]]
    w[7][0, 0, entry[0], entry[1]] += np.float32(unit)
    return w


def weights_dw2_raised(case):
    """the case's weights with tap (0, 2) of channel 11 of L2's depthwise kernel raised by one (forward32_mutated's "dw")"""
    w = [np.array(a, copy=True) for a in build32(case)[2]]
    w[3][0, 2, 11, 0] += 1.0
    return w
