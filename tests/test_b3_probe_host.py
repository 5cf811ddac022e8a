"""Host proof of tests/b3_probe.py: the split model is the exact 3-way split, every exact data family passes its
exactness certificate and really has non-zero entries in the planes it claims, and - the point of it all - a kernel
that loses any ONE of the six plane products would be caught: exactly (a difference in every column tile and k block
of some exact family) and by the bounded per-entry check on full mantissas (more than 10 x the cap).  No GPU."""
import numpy as np
import pytest

import b3_probe as bp

DS = (200, 208)


def _fx(name, layout, D, room=False):
    return bp.family(name, layout, 2 * D + 7, D, D, seed=1, room=room)      # every k with both signs, a ragged end


def test_split_model():
    rng = np.random.default_rng(0)
    x = np.concatenate([(rng.standard_normal(40000) * np.exp(rng.uniform(-20, 20, 40000))).astype(np.float32),
                        np.float32([0.0, -0.0, 1.0, -2.0, 1 + 2.0 ** -7 + 2.0 ** -15 + 2.0 ** -23, 1 + 2.0 ** -8,
                                    1 + 3 * 2.0 ** -8, 0.99999994])])
    hi, mid, lo = bp.split3(x)                                # asserts hi + mid + lo == x in float64
    for p in (hi, mid, lo):                                   # each plane is a bf16 number
        assert not (p.view(np.uint32) & np.uint32(0xffff)).any()
    nz = x != 0
    ulp_hi = 2.0 ** (np.frexp(np.where(nz, hi, 1).astype(np.float64))[1] - 8)        # 8 significant bits
    r = x.astype(np.float64) - hi
    assert (np.abs(r) <= ulp_hi / 2)[nz].all()                # round to nearest: |x - hi| <= ulp(hi) / 2
    assert (np.abs(r - mid) <= np.abs(r) * 2.0 ** -8 + 1e-300).all()
    assert (np.abs(x.astype(np.float64)) * 2.0 ** -16 >= np.abs(lo) * (1 - 2.0 ** -7))[nz].all()
    # ties go to even: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert bp.bf16(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8])).tolist() == [1.0, 1 + 2.0 ** -6]
    # the single products of the issue text are exact in the six-product sum
    one = np.float32([[1 + 2.0 ** -7 + 2.0 ** -15 + 2.0 ** -23]])
    assert bp.six_products(one, np.float32([[0.5]]))[0, 0] == float(one[0, 0]) * 0.5
    assert bp.six_products(np.float32([[-2.0]]), one)[0, 0] == -2.0 * float(one[0, 0])
    m = np.float32([[1 + 2.0 ** -10]])
    assert bp.six_products(m, m)[0, 0] == float(m[0, 0]) ** 2


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("layout,room", [("one", False), ("one", True), ("sparse", False), ("sparse4", False)])
@pytest.mark.parametrize("name", bp.EXACT)
def test_families_are_exact_and_use_their_planes(name, layout, room, D):
    fx = _fx(name, layout, D, room)
    nnz = (fx.A != 0).sum(1)
    if layout == "one":
        r = np.arange(fx.A.shape[0])
        assert (nnz == 1).all() and (fx.A[r, r % D] != 0).all()
        assert {(k, s) for k, s in zip(r % D, np.sign(fx.A[r, r % D]))} == {(k, s) for k in range(D) for s in (-1.0, 1.0)}
    elif layout == "sparse4":                                 # two entries of opposite sign in one group of four per k block
        assert (nnz == 2 * ((D + bp.KB - 1) // bp.KB)).all()
        g = fx.A.reshape(fx.A.shape[0], D // 4, 4)
        used = (g != 0).any(2)
        assert ((g > 0).sum(2)[used] == 1).all() and ((g < 0).sum(2)[used] == 1).all()
        for k0 in range(0, D, bp.KB):
            assert ((fx.A[:, k0:k0 + bp.KB] != 0).sum(1) == 2).all()
        bp.certify(fx.A, 2 * fx.W, fx.live)                   # room for an instruction entry of 2 on the weight side
    else:
        assert nnz.min() >= 16 and nnz.max() <= 32
        for k0 in range(0, D, bp.KB):                         # every row reaches into every k block
            assert (fx.A[:, k0:k0 + bp.KB] != 0).any(1).all()
    want = bp.certify(fx.A, fx.W, fx.live)
    assert np.array_equal(want, bp.six_products(fx.A, fx.W))              # six products, not nine, make the result
    assert (want > 0).any() and (want < 0).any()
    b, nbr = bp.addends(np.random.default_rng(D), fx.A.shape[0], D)
    if room or layout == "sparse":                            # the fixtures that leave room for bias and neighbour sum
        bp.certify(fx.A, fx.W, fx.live, extra=(b[None, :], nbr))
    na, nw = bp.planes_in_use(fx)
    want_a = {"a3_whi": (1, 1, 1), "ahi_w3": (1, 0, 0), "mid_mid": (1, 1, 0)}[name]
    want_w = {"a3_whi": (1, 0, 0), "ahi_w3": (1, 1, 1), "mid_mid": (1, 1, 0)}[name]
    n_a, n_w = int((fx.A != 0).sum()), fx.W.size
    for p in range(3):                                        # a plane in use is non-zero in EVERY non-zero entry
        assert na[p] == want_a[p] * n_a, (name, "A", p, na)
        assert nw[p] == want_w[p] * n_w, (name, "W", p, nw)


def test_certificate_rejects_what_is_not_exact():
    fx = _fx("full_full", "one", 200)
    with pytest.raises(AssertionError):
        bp.certify(fx.A, fx.W, fx.live)
    fx = _fx("a3_whi", "one", 200)
    with pytest.raises(AssertionError):                       # a full mantissa leaves no room for an addend
        bp.certify(fx.A, fx.W, fx.live, extra=(np.ones((1, 200), dtype=np.float32),))
    with pytest.raises(AssertionError):                       # wrong claim about the live terms
        bp.certify(fx.A, fx.W, ("hh", "mh"))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("term", list(bp.TERMS))
def test_every_lost_product_shows_exactly(term, D):
    """For each of the six products some exact family differs from the float64 result, when that product is left
    out, in at least one entry of every (k block, column tile) - in the "one" layout row m is the k = m mod D."""
    hit = []
    for name in bp.EXACT:
        if term not in bp.LIVE[name]:
            continue
        fx = _fx(name, "one", D)
        diff = bp.six_products(fx.A, fx.W, drop=term) != bp.certify(fx.A, fx.W, fx.live)
        kb = (np.arange(fx.A.shape[0]) % D) // bp.KB
        cells = {(b, t) for b in range((D + bp.KB - 1) // bp.KB) for t in range((D + 15) // 16)
                 if diff[kb == b][:, 16 * t:16 * t + 16].any()}
        if len(cells) == ((D + bp.KB - 1) // bp.KB) * ((D + 15) // 16):
            hit.append(name)
        fs = _fx(name, "sparse", D)                           # and in the accumulating layout: every row, every tile
        ds = bp.six_products(fs.A, fs.W, drop=term) != bp.certify(fs.A, fs.W, fs.live)
        assert all(ds[:, 16 * t:16 * t + 16].any() for t in range((D + 15) // 16)), (name, term)
    assert hit, term


@pytest.mark.parametrize("rz", [False, True], ids=["nearest", "toward_zero"])
def test_bounded_check_separates_the_mutants(rz):
    """full_full, one non-zero per row: the faithful model (fp32 accumulation in the kernel's order, the accumulator
    rounding to nearest or - what the MI355X's figures match - toward zero) stays within the project's cap of 4e-7 per
    entry; every mutant exceeds ten times the cap."""
    fx = _fx("full_full", "one", 200)
    clean64 = bp.entry_error(bp.six_products(fx.A, fx.W), fx.A, fx.W)
    clean32 = bp.entry_error(bp.six_products(fx.A, fx.W, order=bp.KERNEL_ORDER, rz=rz), fx.A, fx.W)
    print("full_full one-non-zero rows: e = %.3g (float64 accumulation), %.3g (fp32, kernel order)" % (clean64, clean32))
    assert clean64 <= clean32 <= bp.E_CAP
    for term in bp.TERMS:
        e = bp.entry_error(bp.six_products(fx.A, fx.W, drop=term, order=bp.KERNEL_ORDER, rz=rz), fx.A, fx.W)
        print("  without %s: e = %.3g = %.1f x cap" % (term, e, e / bp.E_CAP))
        assert e > 10 * bp.E_CAP, term
