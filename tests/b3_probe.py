"""Host model of the bf16x3 scheme and the data that makes its kernels exactly checkable (numpy only).

The scheme (csrc/gnnrag_common.h: split3; header of csrc/tables_b3.hip): every fp32 operand is split EXACTLY into three
bf16 planes hi + mid + lo, rounding to nearest, and six of the nine plane products are accumulated in fp32:
hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid (issued smallest first).  mid*lo, lo*mid and lo*lo are left out.

``split3`` / ``six_products`` restate that on the host.  The data families below put non-zero middle and low planes
under the kernels in a way that still has ONE right answer: every live plane product of an output entry is a multiple
of a unit u and the absolute values of all its terms sum to less than 2**24 * u, so every partial sum in every order is
a multiple of u below 2**24 * u - an fp32 number - and an fp32 accumulation cannot round.  A kernel that loses,
misplaces or doubles a plane product then differs from the float64 result by at least u in that entry.
``certify`` asserts these conditions for the very operands a test uses.

Families (``family``): the planes they drive and the terms that are live (all others are exactly zero)
    a3_whi     A: three planes, W: high plane only (+-2**j)            hh mh lh
    ahi_w3     A: high plane only,  W: three planes                     hh hm hl
    mid_mid    both +-2**i (1 + m 2**-10): high and middle planes       hh hm mh mm
    full_full  full mantissas on both sides (NOT exact: bounded check)  all six
Layouts: "one" - one non-zero per row of A at k = row mod K, sign changing every K rows (every k, every k block, the
padding tail and both signs); "sparse" - 3-4 non-zeros in every k block of 32 (2 in the last), so that planes
accumulate across k blocks, with magnitudes on a coarser grid so that the certificate still holds; "sparse4" - for the
relation tables, whose weight operand is scaled by an instruction entry of up to 2 (half the room): in every k block one
group of four consecutive k with two non-zeros of opposite sign (the 2:4 sparse instruction picks by sign).
"""
import collections

import numpy as np

f32, f64 = np.float32, np.float64

TERMS = collections.OrderedDict([("hh", (0, 0)), ("hm", (0, 1)), ("mh", (1, 0)), ("hl", (0, 2)), ("lh", (2, 0)),
                                 ("mm", (1, 1))])          # name -> (plane of A, plane of W), as the header lists them
UNUSED = ((1, 2), (2, 1), (2, 2))
KERNEL_ORDER = ("mm", "lh", "hl", "mh", "hm", "hh")        # issue order inside a k block (PA / PB in tables_b3.hip)
KB = 32                                                    # k block of v_mfma_f32_16x16x32_bf16
E_CAP = 4e-7                                               # the project's per-entry cap (test_gpu_dense_forms.py)
LIVE = {"a3_whi": ("hh", "mh", "lh"), "ahi_w3": ("hh", "hm", "hl"), "mid_mid": ("hh", "hm", "mh", "mm"),
        "full_full": tuple(TERMS)}
EXACT = ("a3_whi", "ahi_w3", "mid_mid")


def bf16(x):
    """fp32 -> nearest bf16 (ties to even) on the bit pattern, returned as fp32."""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    r = (b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(f32)


def split3(x):
    """The kernel's split: hi = bf16(x), r = x - hi, mid = bf16(r), q = r - mid, lo = bf16(q), remainders in fp32."""
    x = np.ascontiguousarray(x, dtype=f32)
    hi = bf16(x)
    r = (x - hi).astype(f32)
    mid = bf16(r)
    q = (r - mid).astype(f32)
    lo = bf16(q)
    assert np.array_equal(hi.astype(f64) + mid.astype(f64) + lo.astype(f64), x.astype(f64)), "split3 is not exact"
    return hi, mid, lo


def _one_k(A):
    """Column of the single non-zero of every row, or None when some row holds more than one."""
    nz = A != 0
    return np.argmax(nz, 1) if nz.sum(1).max(initial=0) <= 1 else None


def rows_matmul(A, W, dt=f64):
    """A @ W.T in ``dt`` (float64); rows with one non-zero take the gather a * W[:, k] (same value, no M*N*K product)."""
    A, W = np.asarray(A), np.asarray(W)
    k = _one_k(A)
    if k is None:
        return A.astype(dt) @ W.astype(dt).T
    a = A[np.arange(A.shape[0]), k].astype(dt)
    return a[:, None] * W.astype(dt).T[k]


def _toward_zero(x):
    """float64 -> fp32, rounding toward zero."""
    y = x.astype(f32)
    over = np.abs(y.astype(f64)) > np.abs(x)
    y[over] = np.nextafter(y[over], f32(0))
    return y


def six_products(A, W, drop=None, order=None, rz=False):
    """The plane-product sum of A [M, K] and W [N, K] -> [M, N].  ``drop``: a term name to leave out (a mutant).
    ``order=None``: float64 accumulation.  ``order=<term names>``: fp32 accumulation as the kernels do it - k blocks of
    32 outermost, inside a block one MFMA per term in this order (the 32 products of one MFMA are summed in float64);
    ``rz``: the accumulator rounds toward zero instead of to nearest (what the MI355X's results match)."""
    pa, pw = split3(A), split3(W)
    names = [t for t in (order or TERMS) if t != drop]
    if order is None:
        out = np.zeros((A.shape[0], W.shape[0]), dtype=f64)
        for t in names:
            out += rows_matmul(pa[TERMS[t][0]], pw[TERMS[t][1]])
        return out
    rnd = _toward_zero if rz else (lambda x: x.astype(f32))
    k = _one_k(np.asarray(A))
    acc = np.zeros((A.shape[0], W.shape[0]), dtype=f32)
    for k0 in range(0, A.shape[1], KB):
        rows = slice(None) if k is None else np.flatnonzero((k >= k0) & (k < k0 + KB))      # the others add zeros
        for t in names:
            i, j = TERMS[t]
            acc[rows] = rnd(acc[rows].astype(f64) + pa[i][rows, k0:k0 + KB].astype(f64) @ pw[j][:, k0:k0 + KB].astype(f64).T)
    return acc.astype(f64)


def grid(x):
    """Value of the lowest set mantissa bit of every fp32 entry (inf for zeros): x is a multiple of grid(x)."""
    m, e = np.frexp(np.asarray(x, dtype=f32).astype(f64))
    mi = np.abs(np.round(np.ldexp(m, 24))).astype(np.int64)
    low = (mi & -mi).astype(f64)
    with np.errstate(divide="ignore"):
        return np.where(mi == 0, np.inf, np.ldexp(low, e - 24))


def _is_multiple(x, u):
    q = np.asarray(x, dtype=f64) / u
    return bool(np.all(q == np.round(q)))


def certify(A, W, live, extra=()):
    """The exactness certificate of the product A @ W.T (+ the [M, N]-broadcastable fp32 addends ``extra``, e.g. bias
    and neighbour sum).  Asserts
      1. the three unused plane products are zero for every pair of operand entries that meets, and so is every term
         outside ``live``;
      2. every plane entry is a multiple of its operand's unit and so every term of an output entry a multiple of
         u[m, n] (one non-zero per row: the units of the two entries that meet; else row minimum times row minimum);
      3. sum |terms| (+ |extra|) < 2**24 * u[m, n];
      4. the float64 result equals its fp32 rounding.
    Returns the float64 result (with ``extra`` added)."""
    A, W = np.asarray(A, dtype=f32), np.asarray(W, dtype=f32)
    k = _one_k(A)
    pw = split3(W)
    gw = np.minimum.reduce([grid(p) for p in pw])
    if k is not None:                                         # one non-zero per row: work on that column of values
        a = A[np.arange(A.shape[0]), k]
        pa = split3(a)
        mm = lambda x, Y, dt=f64: x.astype(dt)[:, None] * Y.astype(dt).T[k]
        u = np.minimum.reduce([grid(p) for p in pa])[:, None] * gw.T[k]
        u = np.where(np.isfinite(u), u, 1.0)                  # an empty row / a zero weight: the term is 0
    else:
        a = A
        pa = split3(A)
        mm = lambda X, Y, dt=f64: X.astype(dt) @ Y.astype(dt).T
        ga = np.minimum.reduce([grid(p) for p in pa])
        gar, gwr = (np.where(np.isfinite(g.min(1)), g.min(1), 1.0)[:, None] for g in (ga, gw))      # (an empty row: 0)
        u = gar * gwr.T
        for p, g in zip(pa + pw, (gar,) * 3 + (gwr,) * 3):
            assert _is_multiple(p, g)
    ind = lambda p: (p != 0).astype(f32)
    dead = list(UNUSED) + [TERMS[t] for t in TERMS if t not in live]
    for i, j in dead:
        meets = mm(ind(pa[i]), ind(pw[j]), f32)               # counts <= K: exact in fp32
        assert meets.max(initial=0) == 0, "plane product (%d, %d) is not zero" % (i, j)
    S = mm(sum(np.abs(p).astype(f64) for p in pa), sum(np.abs(p).astype(f64) for p in pw))
    want = mm(a, W)
    for x in extra:
        x = np.asarray(x, dtype=f32).astype(f64)
        assert _is_multiple(np.broadcast_to(x, u.shape), u), "an addend is off the grid"
        S = S + np.abs(x)
        want = want + x
    assert (S < 2.0 ** 24 * u).all(), "partial sums can exceed 24 bits: max S / (2^24 u) = %g" % (S / (2.0 ** 24 * u)).max()
    assert _is_multiple(want, u)
    assert np.array_equal(want, want.astype(f32).astype(f64))
    return want


# ---- values ------------------------------------------------------------------------------------------------------------

def _sign(rng, shape):
    return rng.choice(np.array([-1.0, 1.0]), size=shape)


def mant3(rng, shape, bits, exps=(0,)):
    """Positive values whose three planes are all non-zero.  bits = 24: (1 + f 2**-23) in [1, 1.9), f odd - a full
    24-bit mantissa; bits = 18: on the 2**-18 grid in [0.5, 1) with the last bit set.  Times 2**e, e from ``exps``."""
    n = int(np.prod(shape))
    out = np.zeros(n, dtype=f64)
    todo = np.arange(n)
    for _ in range(200):
        if bits == 24:
            v = 1.0 + (2 * rng.integers(0, int(0.45 * 2 ** 23), size=todo.size) + 1) * 2.0 ** -23
        else:
            v = (2 ** 17 + 2 * rng.integers(0, 2 ** 16, size=todo.size) + 1) * 2.0 ** -18
        hi, mid, lo = split3(v.astype(f32))
        ok = (mid != 0) & (lo != 0)
        out[todo[ok]] = v[ok]
        todo = todo[~ok]
        if todo.size == 0:
            break
    assert todo.size == 0
    return (out * 2.0 ** rng.choice(np.array(exps), size=n)).reshape(shape).astype(f32)


def hi_only(rng, shape, exps):
    """+-2**j: the high plane alone."""
    return (_sign(rng, shape) * 2.0 ** rng.choice(np.array(exps), size=shape)).astype(f32)


def mid_form(rng, shape, even, exp):
    """+-2**exp (1 + m 2**-10), m not a multiple of 8 (a non-zero middle plane, an empty low one); ``even``: m even and
    <= 254 (values on the 2**-9 grid below 1.25: room for a sum of ~25 products)."""
    m = rng.integers(1, 128 if even else 1024, size=shape)
    m = np.where(m % (4 if even else 8) == 0, m + 1, m)
    m = 2 * m if even else m
    return (_sign(rng, shape) * (1.0 + m * 2.0 ** -10) * 2.0 ** exp).astype(f32)


def layout_mask(rng, layout, M, K):
    """[M, K] bool positions of A's non-zeros and their signs ([M, 1], [M, K], or None: random)."""
    r = np.arange(M)
    if layout == "one":
        mask = np.zeros((M, K), dtype=bool)
        mask[r, r % K] = True
        return mask, np.where((r // K) % 2 == 0, 1.0, -1.0)[:, None]
    mask = np.zeros((M, K), dtype=bool)
    if layout == "sparse4":
        assert K % 4 == 0
        sign = np.zeros((M, K))
        for k0 in range(0, K, KB):
            g = k0 + 4 * rng.integers(0, min(KB, K - k0) // 4, size=M)
            pos = np.argsort(rng.random((M, 4)), 1)[:, :2]     # two distinct positions of the group, signs + and -
            s = _sign(rng, M)
            for j in range(2):
                mask[r, g + pos[:, j]] = True
                sign[r, g + pos[:, j]] = s if j == 0 else -s
        return mask, sign
    assert layout == "sparse"
    score = rng.random((M, K))
    for k0 in range(0, K, KB):
        w = min(KB, K - k0)
        cnt = rng.integers(3, 5, size=M) if w == KB else np.full(M, min(2, w))
        thr = np.sort(score[:, k0:k0 + w], 1)[r, cnt - 1]
        mask[:, k0:k0 + w] = score[:, k0:k0 + w] <= thr[:, None]
    return mask, None


Fixture = collections.namedtuple("Fixture", "name layout A W live")


def family(name, layout, M, K, N, seed=0, room=False):
    """Operands A [M, K] (in ``layout``) and W [N, K] (dense) of a family.  ``room``: the "one" layout also takes the
    coarser grids of the sparse one, which leaves headroom for addends (bias, neighbour sum, a second instruction)."""
    rng = np.random.default_rng([seed, M, K, N, len(name), len(layout)])
    mask, rsign = layout_mask(rng, layout, M, K)
    many = layout != "one"                                    # rows that accumulate several products
    coarse = room or many
    sgn = (_sign(rng, (M, K)) if rsign is None else np.broadcast_to(rsign, (M, K)))[mask]
    n = int(mask.sum())                                       # A's values are drawn for its non-zeros only
    if name == "a3_whi":
        a = mant3(rng, n, 18 if coarse else 24, (0,) if coarse else (-1, 0))
        W = hi_only(rng, (N, K), (0, 1) if many else (-1, 0, 1))
    elif name == "ahi_w3":
        a = np.abs(hi_only(rng, n, (0, 1) if many else (-1, 0, 1)))
        W = mant3(rng, (N, K), 18 if coarse else 24, (0,) if coarse else (-1, 0)) * _sign(rng, (N, K))
    elif name == "mid_mid":
        a = np.abs(mid_form(rng, n, many, 0))
        W = mid_form(rng, (N, K), many, -1) if coarse else \
            mid_form(rng, (N, K), False, -1) * 2.0 ** rng.integers(0, 2, size=(N, K))
    else:
        assert name == "full_full" and layout == "one"
        a = np.abs(rng.standard_normal(n))
        W = rng.standard_normal((N, K)) / np.sqrt(K)
    A = np.zeros((M, K), dtype=f32)
    A[mask] = a * sgn
    return Fixture(name, layout, A, np.ascontiguousarray(W, dtype=f32), LIVE[name])


def planes_in_use(fx):
    """(non-zero entries per plane of A, per plane of W)."""
    return tuple(int((p != 0).sum()) for p in split3(fx.A)), tuple(int((p != 0).sum()) for p in split3(fx.W))


def addends(rng, M, N):
    """Bias [N] and neighbour sum [M, N]: small integers (on every grid the room / sparse fixtures use)."""
    return rng.integers(-2, 3, size=N).astype(f32), rng.integers(-2, 3, size=(M, N)).astype(f32)


def entry_error(got, A, W):
    """e = |got - want64| / (|A| |W|^T) per entry (want64 = the float64 product), entries with S = 0 excluded."""
    want = rows_matmul(A, W)
    S = rows_matmul(np.abs(A), np.abs(W))
    live = S > 0
    return float((np.abs(np.asarray(got, dtype=f64) - want)[live] / S[live]).max())
