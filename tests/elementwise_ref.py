"""Host references, bounds and cases for the flat kernels of tubedetr_amd/csrc/elementwise.hip, shared by
tests/test_elementwise_cpu.py (the cases are well posed) and tests/test_elementwise_gpu.py (the kernels).  numpy / torch on
the CPU only.  bf16 values travel as uint16 bit patterns in numpy and as torch.bfloat16 on the device."""
import numpy as np
import torch

U = 2.0 ** -24  # one fp32 rounding unit
VEC = {"f32": 4, "bf16": 8}  # elements per 16-byte access
GRID_CAP = 4096  # workgroups of 256 lanes


def sizes(dt):
    """1, VEC-1, VEC, VEC+1, several workgroups with a tail, and one vector plus a 3-element tail past the grid cap."""
    v = VEC[dt]
    return [1, v - 1, v, v + 1, 257 * v + 3, GRID_CAP * 256 * v + v + 3]


# ------------------------------------------------------------------------------------------------------------- bfloat16
def f32_to_bf16_bits(x):
    """Round-to-nearest-even float32 -> bf16 bit pattern (uint16); NaN stays NaN (quiet bit set), as f32_to_bf16 in td_common.h."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint16)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_bits_to_f32(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_to(x, dt):
    """float32 array -> the values of dtype ``dt`` as float32 (identity for f32)."""
    x = np.asarray(x, np.float32)
    return x if dt == "f32" else bf16_bits_to_f32(f32_to_bf16_bits(x))


def bits(x, dt):
    """float32 array holding ``dt`` values -> their storage bit pattern (uint32 / uint16)."""
    return np.ascontiguousarray(x, np.float32).view(np.uint32) if dt == "f32" else f32_to_bf16_bits(x)


def half_ulp_bf16(x):
    """Half a bf16 ulp at magnitude |x| (float64 array)."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 2.0 ** (e - 8)


# ------------------------------------------------------------------------------------- single-rounding ops (bit-exact)
def add_ref(a, b, dt):
    """bits of a + b computed in float32 and rounded once to ``dt`` (b None: a copy)."""
    return bits(a if b is None else (np.asarray(a, np.float32) + np.asarray(b, np.float32)), dt)


def relu_bwd_ref(dy, y, scale, dt):
    """bits of dy * scale where y > 0, else +0: NaN and both zeros in y block the gradient."""
    with np.errstate(invalid="ignore"):
        r = np.where(np.asarray(y, np.float32) > 0, np.asarray(dy, np.float32) * np.float32(scale), np.float32(0))
    return bits(r, dt)


def relu_cases(n, dt, seed=0):
    """dy, y (float32 arrays of ``dt`` values): y cycles through +0, -0, the smallest positive subnormal, a negative value,
    NaN, and ordinary positives / negatives."""
    rng = np.random.default_rng(seed + n)
    dy = round_to(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n), dt)
    tiny = np.uint32(1).view(np.float32) if dt == "f32" else bf16_bits_to_f32(np.array([1], np.uint16))[0]
    special = np.array([0.0, -0.0, tiny, -tiny, np.nan, -1.5, 2.0, 1e-3], np.float32)
    y = np.where(np.arange(n) % 3 == 0, special[(np.arange(n) // 3) % len(special)], rng.standard_normal(n)).astype(np.float32)
    return dy, round_to(y, dt)


# ------------------------------------------------------------------------------------------------------------- dropout
# include/tubedetr_hip.h: keep(seed, element index) = hash32(element index * golden + seed) >= p * 2^32; with a dropout
# counter the seed is re-keyed by a hash of (seed, counter).
GOLDEN = np.uint32(0x9E3779B1)


def mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def effective_seed(seed, counter=None):
    """counter None: the seed as passed; else mix32(mix32(seed ^ 0xA511E9B3) + counter * 0xC2B2AE3D)."""
    seed = np.uint32(seed & 0xFFFFFFFF)
    if counter is None:
        return seed
    with np.errstate(over="ignore"):
        a = mix32(np.array([seed ^ np.uint32(0xA511E9B3)], np.uint32))
        return mix32(a + np.array([counter & 0xFFFFFFFF], np.uint32) * np.uint32(0xC2B2AE3D))[0]


def hash32(seed, n):
    """hash32(seed, idx) for idx in [0, n) (uint32 array)."""
    with np.errstate(over="ignore"):
        return mix32(np.arange(n, dtype=np.uint32) * GOLDEN + np.uint32(seed))


def threshold(p):
    """uint32(p * 2^32), at least 1 for p > 0; an element is kept when its hash is >= the threshold."""
    if p <= 0:
        return 0
    return max(1, int(float(np.float32(p)) * 4294967296.0))


def dropout_keep(n, p, seed, counter=None):
    return hash32(effective_seed(seed, counter), n) >= np.uint32(threshold(p))


def dropout_scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


# ---------------------------------------------------------------------------------------------------------------- GELU
def _erf64(x):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


def gelu64(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + _erf64(x / np.sqrt(2.0)))


def gelu_grad64(x):
    """d/dx x*Phi(x) = Phi(x) + x*phi(x)."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return 0.5 * (1.0 + _erf64(x / np.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def gelu_emul32(x):
    """The erf form in float32, one rounding per operation, with a correctly rounded erff."""
    F = np.float32
    x = np.asarray(x, F)
    erf = _erf64((x * F(0.70710678118654752)).astype(np.float64)).astype(F)
    return F(0.5) * x * (F(1) + erf)


def gelu_grad_emul32(dy, x):
    F = np.float32
    dy, x = np.asarray(dy, F), np.asarray(x, F)
    erf = _erf64((x * F(0.70710678118654752)).astype(np.float64)).astype(F)
    with np.errstate(over="ignore"):
        ex = np.exp((F(-0.5) * x * x).astype(np.float64)).astype(F)
    return dy * (F(0.5) * (F(1) + erf) + x * F(0.3989422804014327) * ex)


def gelu_tanh64(x):  # mutant: the tanh approximation
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def gelu_grad_no_pdf64(x):  # mutant: a backward without the x*phi(x) term
    x = np.asarray(x, np.float64)
    return 0.5 * (1.0 + _erf64(x / np.sqrt(2.0)))


# The error unit is absolute: 1 + erf cancels for negative x in any fp32 erf-form GELU.  c = 4 x the worst err/unit of the
# numpy-float32 emulations above against float64 over gelu_inputs("f32", ...) (tests/test_elementwise_cpu.py recomputes them).
GELU_FWD_MEASURED, C_GELU_FWD = 1.56, 6.3  # units of 2^-24 |x|
GELU_BWD_MEASURED, C_GELU_BWD = 1.18, 4.8  # units of 2^-24 |dy| (1 + |x|)
BF16_MAX = float(bf16_bits_to_f32(np.array([0x7F7F], np.uint16))[0])  # 3.3895e38, finite in float32 as well


def gelu_inputs(dt, n, seed=0):
    """x, dy (float32 arrays of ``dt`` values) of length n: a dense grid over [-12, 12], +-0, values around +-1e-4, the
    largest finite bf16, repeated to length n; dy spans 1e-6 .. 1e2 with both signs."""
    grid = np.linspace(-12.0, 12.0, 4801)
    extra = np.array([0.0, -0.0, 1e-4, -1e-4, 0.5e-4, -0.5e-4, 2e-4, -2e-4, BF16_MAX, -BF16_MAX])
    base = np.concatenate([extra, grid])
    x = round_to(np.resize(base, n), dt)
    rng = np.random.default_rng(seed)
    dy = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 2, n)
    return x, round_to(dy, dt)


def gelu_fwd_bound(x, dt):
    """Per element: C * 2^-24 * |x| (+ half a bf16 ulp of the result)."""
    x = np.asarray(x, np.float64)
    b = C_GELU_FWD * U * np.abs(x)
    return b if dt == "f32" else b + half_ulp_bf16(np.abs(gelu64(x)) + b)


def gelu_bwd_bound(dy, x, dt):
    """Per element: C * 2^-24 * |dy| * (1 + |x|) (+ half a bf16 ulp of the result)."""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    b = C_GELU_BWD * U * np.abs(dy) * (1.0 + np.abs(x))
    return b if dt == "f32" else b + half_ulp_bf16(np.abs(dy * gelu_grad64(x)) + b)


# -------------------------------------------------------------------------------------------------------------- colsum
# (rows, cols, ld) in bf16; the fp32 vector cases use cols / 2.  Vector route: cols and ld multiples of 16 bytes.
COLSUM_VECTOR = [(1, 8, 8), (7, 264, 264), (65, 264, 264), (129, 264, 264), (1000, 24, 24)]
COLSUM_GENERIC = [(130, 7, 7), (9, 300, 300), (64, 12, 12)]  # bf16: no multiple of 8
COLSUM_GENERIC_F32 = [(130, 7, 7), (9, 301, 301), (64, 13, 13)]  # fp32: no multiple of 4
COLSUM_LD = [(65, 16, 40), (65, 7, 9)]


def colsum_shapes(dt):
    vec = [(r, c if dt == "bf16" else c // 2, l if dt == "bf16" else l // 2) for r, c, l in COLSUM_VECTOR]
    return [("vector",) + s for s in vec] + [("generic",) + s for s in (COLSUM_GENERIC if dt == "bf16" else COLSUM_GENERIC_F32)] + [("vector", 65, 16, 40), ("generic", 65, 7, 9)]


def colsum_route(cols, ld, dt):
    return "vector" if cols % VEC[dt] == 0 and ld % VEC[dt] == 0 else "generic"


def colsum_case(rows, cols, ld, dt, seed=0):
    """-> g [rows, ld] float32 array of ``dt`` values (the columns >= cols are padding that must not be summed), the float64
    column sums, and the per-column bound rows * 2^-24 * sum_r |g[r, c]|."""
    rng = np.random.default_rng(seed + rows * 1000 + cols)
    g = round_to(rng.standard_normal((rows, ld)) * 10.0 ** rng.integers(-2, 2, (rows, ld)), dt).reshape(rows, ld)
    g[:, cols:] = 777.0
    g64 = g[:, :cols].astype(np.float64)
    return g, g64.sum(0), rows * U * np.abs(g64).sum(0)


# ----------------------------------------------------------------------------------------------------------- LayerNorm
LN_ROWS = [1, 3, 4, 5, 33]
LN_COLS = [1, 63, 64, 65, 256, 768, 1000, 1024]
LN_TOL = {"f32": 2e-5, "bf16": 1.2e-2}  # per element, relative to the row's largest reference magnitude


def ln_route(cols, dt):
    return "vector" if dt == "bf16" and cols in (256, 768) else "generic"


def ln_case(rows, cols, dt, seed=0):
    rng = np.random.default_rng(seed + 100 * rows + cols)
    mk = lambda *s: round_to(rng.standard_normal(s), dt).reshape(s)
    x, r, dy, extra = mk(rows, cols), mk(rows, cols), mk(rows, cols), mk(rows, cols)
    gamma = (1.0 + 0.5 * rng.standard_normal(cols)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(cols)).astype(np.float32)
    return x, r, gamma, beta, dy, extra


def ln_fwd64(x, r, gamma, beta, eps):
    """-> y, s (= x + r), mean, rstd in float64."""
    s = x.astype(np.float64) + (0.0 if r is None else r.astype(np.float64))
    mean = s.mean(1)
    var = ((s - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + eps)
    return (s - mean[:, None]) * rstd[:, None] * gamma.astype(np.float64) + beta.astype(np.float64), s, mean, rstd


def ln_bwd64(dy, s, mean, rstd, gamma, extra):
    """-> ds (+ extra), dgamma, dbeta in float64 from the saved sum / mean / rstd."""
    dy, s, gamma = dy.astype(np.float64), s.astype(np.float64), gamma.astype(np.float64)
    xh = (s - mean[:, None]) * rstd[:, None]
    dg = dy * gamma
    c1, c2 = dg.mean(1), (dg * xh).mean(1)
    ds = rstd[:, None] * (dg - c1[:, None] - xh * c2[:, None])
    if extra is not None:
        ds = ds + extra.astype(np.float64)
    return ds, (dy * xh).sum(0), dy.sum(0)


def row_rel_err(got, ref):
    """max over the elements of |got - ref| / (the row's largest |ref|)."""
    scale = np.maximum(np.abs(ref).max(axis=-1, keepdims=True), 1e-30)
    return float((np.abs(got.astype(np.float64) - ref) / scale).max()) if ref.size else 0.0
