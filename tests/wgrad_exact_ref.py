"""Plain references and inputs for the bit-exact weight-gradient tests (test_wgrad_exact_cpu.py, test_wgrad_exact_gpu.py).  No GPU needed.

Why a weight gradient can be compared with torch.equal: both operands come from a dyadic integer grid, g = a / 2^p and x = b / 2^q with
integers |a| <= A, |b| <= B <= 127 (exact in bf16, the implicit-bit corner left alone).  Every product and every partial sum is then an integer
multiple of 2^-(p+q), and as long as M_total * A * B < 2^24 - M_total = the number of products that can land in one output element: all
reduction rows, the rows of every accumulating job onto the same dW, one more for a value the output already holds - none of them needs more
than 24 significant bits: every fp32 addition is exact, in any order and any rounding mode, inside an MFMA or as an atomic.  A per-channel
power-of-two factor (FrozenBN scale) multiplies every partial sum of an element alike and changes exponents only.  The condition is a property
of the inputs, asserted by check_exactness_condition for every case; it is no tolerance."""
import torch

SHIFT = 4  # p = q: every operand is a multiple of 1/16, every product of 1/256
BOUNDS = (63, 31, 15, 7, 3, 1)  # A = B, largest first: as many mantissa bits as the row count leaves


def check_exactness_condition(M_total, A, B):
    """fp32 sums of M_total products of grid values bounded by A and B are exact in any order"""
    assert 1 <= A <= 127 and 1 <= B <= 127, (A, B)
    assert M_total >= 1 and M_total * A * B < 2 ** 24, f"{M_total} products of |a| <= {A}, |b| <= {B} can need more than 24 bits"


def pick_bound(M_total):
    """the largest grid bound A = B of BOUNDS under which M_total products sum exactly"""
    for a in BOUNDS:
        if M_total * a * a < 2 ** 24:
            check_exactness_condition(M_total, a, a)
            return a
    raise AssertionError(f"no grid for {M_total} products")


def grid_tensor(shape, gen, bound, shift=SHIFT, zero_frac=0.0):
    """fp32 tensor of a / 2^shift, integer a uniform in [-bound, bound]; a fraction zero_frac of the elements is zeroed on top"""
    a = torch.randint(-bound, bound + 1, tuple(shape), generator=gen, dtype=torch.int64)
    if zero_frac > 0:
        a = a * (torch.rand(tuple(shape), generator=gen) >= zero_frac)
    return a.to(torch.float32) / float(2 ** shift)


def fill_zeros_(t, value):
    """zeros of t (a view is fine) -> value, in place"""
    t.masked_fill_(t == 0, value)
    return t


def gradient_rows(shape, gen, bound):
    """g [..., channels]: dense, both signs; the first and the last reduction row are non-zero in every channel"""
    g = grid_tensor(shape, gen, bound)
    rows = g.view(-1, shape[-1])
    one = 1.0 / 2 ** SHIFT
    fill_zeros_(rows[0], one)
    fill_zeros_(rows[-1], -one)
    return g


def activation_nhwc(shape, gen, bound):
    """x [N, H, W, C]: about half zeros (post-ReLU), but the first and last image row and column of every frame non-zero - and with them the
    first and the last row of the flattened tensor"""
    x = grid_tensor(shape, gen, bound, zero_frac=0.5)
    one = 1.0 / 2 ** SHIFT
    for border in (x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1]):
        fill_zeros_(border, one)
    return x


def activation_rows(shape, gen, bound):
    """x [M, K] of a linear layer: about half zeros, first and last row non-zero"""
    x = grid_tensor(shape, gen, bound, zero_frac=0.5)
    one = 1.0 / 2 ** SHIFT
    fill_zeros_(x[0], one)
    fill_zeros_(x[-1], one)
    return x


def pow2_scale(Co):
    """FrozenBN-like per-channel factors, powers of two varied per channel"""
    return torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.arange(Co) % 4].contiguous()


def conv_out(h, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1


def conv_wgrad_ref(g_nhwc, x_nhwc, R, S, stride, pad, ci_real=None, scale=None):
    """dW [Co, ci_real, R, S] in float64 of y = conv2d(x, W, stride, pad) from g = dL/dy: explicit im2col - per filter tap the slice of the
    zero-padded source that the tap reads, flattened to [M, ci_real], and one float64 matmul against g [M, Co]"""
    N, H, W, C = x_nhwc.shape
    Ng, Ho, Wo, Co = g_nhwc.shape
    assert Ng == N and Ho == conv_out(H, R, stride, pad) and Wo == conv_out(W, S, stride, pad)
    ci = C if ci_real is None else ci_real
    xp = torch.zeros((N, H + 2 * pad, W + 2 * pad, ci), dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W] = x_nhwc[..., :ci].to(torch.float64)
    gt = g_nhwc.to(torch.float64).reshape(-1, Co).t().contiguous()  # [Co, M]
    dW = torch.empty((Co, ci, R, S), dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            tap = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride]  # [N, Ho, Wo, ci]
            dW[:, :, r, s] = gt @ tap.reshape(-1, ci)
    if scale is not None:
        dW *= scale.to(torch.float64).view(-1, 1, 1, 1)
    return dW


def linear_wgrad_ref(g, x):
    """(g^T x [N, K], column sums of g [N]) in float64"""
    g64 = g.to(torch.float64)
    return g64.t() @ x.to(torch.float64), g64.sum(0)


def first_difference(got, ref):
    """None if got and ref hold the same values, else "index: got / ref, n differing" of the first differing element"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    if torch.equal(got, ref):
        return None
    bad = (got != ref).nonzero()
    idx = tuple(bad[0].tolist())
    return f"first difference at {idx}: got {got[idx].item()!r}, reference {ref[idx].item()!r}; {bad.shape[0]} of {ref.numel()} elements differ"


# ------------------------------------------------------------------------------------------------
# The case lists of tests/wgrad_plan_cases.py as operands.  M_total of a case = its reduction rows, plus the rows of an accumulating partner
# onto the same dW, plus one where the test lets the kernel add onto a grid value the output already holds.
def conv_rows(cfg):
    N, Ci, H, W, Co, R, stride, pad = cfg
    return N * conv_out(H, R, stride, pad) * conv_out(W, R, stride, pad)


def conv_operands(cfg, seed, extra=0):
    """(g [N, Ho, Wo, Co], x [N, H, W, Ci], bound) fp32 on the grid for a (N, Ci, H, W, Co, R, stride, pad) geometry; `extra`: products beyond
    the reduction rows that land in an output element"""
    N, Ci, H, W, Co, R, stride, pad = cfg
    bound = pick_bound(conv_rows(cfg) + extra)
    gen = torch.Generator().manual_seed(seed)
    g = gradient_rows((N, conv_out(H, R, stride, pad), conv_out(W, R, stride, pad), Co), gen, bound)
    return g, activation_nhwc((N, H, W, Ci), gen, bound), bound


def linear_operands(M, K, Nn, seed, M_total):
    """(g [M, Nn], x [M, K], bound)"""
    bound = pick_bound(M_total)
    gen = torch.Generator().manual_seed(seed)
    return gradient_rows((M, Nn), gen, bound), activation_rows((M, K), gen, bound), bound


def linear_batch_totals(rows):
    """M_total per job of an EXACT_LINEAR_BATCH-style list: the rows of every job that writes the same dW"""
    total = [r[0] for r in rows]
    for i, r in enumerate(rows):
        if r[5] is not None:
            total[r[5]] += r[0]
    return [total[r[5]] if r[5] is not None else total[i] for i, r in enumerate(rows)]
