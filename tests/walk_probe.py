"""Host side of the exact and per-row tests of the sparse walks (numpy only: no torch, no library).

What is here, in the order the two test files use it:

* ``build_graph``: fact tuples ``(B, N, R, heads, rels, tails)`` whose ROW LENGTHS are placed by hand - a node is given
  ``len0`` facts that arrive at it (direction 0: it is the tail) and ``len1`` that leave it (direction 1: it is the
  head); the other ends go round robin over the question's remaining nodes ("sinks", they may repeat), relations round
  robin over the relations the question is to use.  Placed nodes sit at slots 0, N-1 and on both sides of the 16-node
  set boundaries first.  The tuple is shuffled; the placed lengths are asserted on the shuffled tuple.
* exact data families (``exact_*``) and ``certify``: every term a multiple of u, sum of |terms| < 2^24 u, float64
  result = its fp32 rounding - then every partial sum in every order is an fp32 number and a kernel must return the
  float64 result bit for bit, whatever order it sums in.
* float64 references computed from the caller's tuple (never from the plan): fused walk (both directions or one),
  unfused REASON walk, TypeLayer walk, frontier walk, and the four backward results.
* ``launch_regime`` / ``walk_variant`` / ``hub_form``: small restatements of the host-side launch arithmetic of
  csrc/aggregate.hip (launch_slice, gnnrag_aggregate_fused_variant, hub_dense_on) so that a case can say which regime
  it reaches for a given CU count without a GPU.
* ``walk_model``: a numpy model of the walk's STRUCTURE (merged runs, 4 / 8 / 64-fact steps, node classes, big-node
  list, 16-node sets, column slices, items cut into parts, hub chunks) that takes a flaw as an argument - the proof that
  the fixtures can see what they claim to see (tests/test_walk_probe_host.py).
* ``FUSED_CASES`` ... ``GPU_BACKWARD_CASES``: the case table of tests/test_gpu_walks_exact.py.
"""
import numpy as np

BIG_DEG = 32          # csrc/gnnrag_common.h kBigDeg: LDS walk, rows with more facts in a direction are "big"
TEAM_DEG = 4096       # csrc/aggregate.hip kSliceTeamDeg: a (merged) run longer than this is walked by the workgroup
BIG_CAP = 72          # kSliceBigCap: big nodes of a question kept in LDS; more: lane groups walk everything
HEAVY_DEG = 256       # kHeavyDeg: gather walk, rows with more facts in a direction are hubs, cut in 256-fact chunks
HUB_KS_MAX = 8        # GNNRAG_HUB_KS_MAX
WALK_L2_GATHER, WALK_LDS_16, WALK_LDS_32 = 0, 1, 2
HUB_FORM_NONE, HUB_FORM_DENSE, HUB_FORM_CHUNKED = 0, 1, 2

LIGHT_LADDER = (0, 1, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 31, 32)
MERGED_PAIRS = ((8, 0), (4, 4), (8, 1), (1, 8), (8, 8), (16, 1), (9, 8), (1, 32), (32, 32))   # runs of 8 9 16 17 33 64
MEDIUM_LADDER = (33, 63, 64, 65, 511, 512, 513, 4095, 4096)
HUGE_LADDER = (4097, 4097 + 64 * 16 + 1)


class Graph:
    def __init__(self, name, B, N, R, h, r, t, placed):
        self.name, self.B, self.N, self.R = name, B, N, R
        self.h, self.r, self.t = h, r, t
        self.placed = placed                      # [(question, slot, len0, len1)]
        BN = B * N
        self.len0 = np.bincount(t, minlength=BN)  # facts arriving (direction 0: node is the tail)
        self.len1 = np.bincount(h, minlength=BN)  # facts leaving  (direction 1: node is the head)
        for q, s, l0, l1 in placed:
            assert self.len0[q * N + s] == l0 and self.len1[q * N + s] == l1, (name, q, s, l0, l1)
        key = (h // N) * (R + 1) + r
        self.rel_key, self.row_of = np.unique(key, return_inverse=True)
        self.row_of = self.row_of.reshape(-1)
        self.rel_total = len(self.rel_key)
        self.rel_off = np.searchsorted(self.rel_key // (R + 1), np.arange(B + 1))
        self.rel_cnt = np.diff(self.rel_off)
        self.rel_max = int(self.rel_cnt.max()) if B else 0
        self.q_order = np.argsort(h // N, kind="stable")           # facts question by question (fact order inside)
        self.q_ptr = np.searchsorted((h // N)[self.q_order], np.arange(B + 1))

    @property
    def tuple(self):
        return self.B, self.N, self.R, self.h, self.r, self.t

    @property
    def F(self):
        return len(self.h)

    def big_nodes(self, q):
        """Local slots of question q whose row is longer than BIG_DEG in a direction, ascending."""
        s = slice(q * self.N, (q + 1) * self.N)
        return np.flatnonzero(np.maximum(self.len0[s], self.len1[s]) > BIG_DEG)

    def hubs(self, d):
        return np.flatnonzero((self.len1 if d else self.len0) > HEAVY_DEG)


def _slot_order(N):
    first = [0, N - 1]
    for b in range(16, N - 1, 16):
        first += [b - 1, b]
    seen, out = set(), []
    for s in first + list(range(N)):
        if 0 <= s < N and s not in seen:
            seen.add(s)
            out.append(s)
    return out


def build_graph(name, B, N, R, questions, seed=0):
    """``questions[q]``: dict with ``place`` = [(len0, len1) or (len0, len1, rels0, rels1)] (explicit relation arrays
    per direction or None), ``nrel`` = how many relations the question uses (None: every one of the R), ``sinks`` =
    how many of the unplaced nodes take the other ends (None: all of them), ``extra`` = background facts among the
    sinks.  A question may be ``None``: no facts."""
    rng = np.random.default_rng(seed)
    H, Rl, T, placed = [], [], [], []
    for q in range(B):
        spec = questions[q] if q < len(questions) else None
        if not spec:
            continue
        place = list(spec.get("place", ()))
        order = _slot_order(N)
        assert len(place) < N, name
        slots, rest = order[:len(place)], sorted(order[len(place):])
        ns = spec.get("sinks") or len(rest)
        sinks = np.asarray(rest[:ns], dtype=np.int64)
        nrel = spec.get("nrel") or R
        pool = np.sort(rng.choice(R, nrel, replace=False)) if nrel < R else np.arange(R)
        so, ro = 0, 0

        def other(n):
            nonlocal so
            x = sinks[(so + np.arange(n)) % len(sinks)]
            so += n
            return x

        def rel(n, explicit=None):
            nonlocal ro
            if explicit is not None:
                assert len(explicit) == n
                return np.asarray(explicit, dtype=np.int64)
            x = pool[(ro + np.arange(n)) % len(pool)]
            ro += n
            return x

        for slot, p in zip(slots, place):
            l0, l1 = p[0], p[1]
            r0, r1 = (p[2], p[3]) if len(p) > 2 else (None, None)
            H += [other(l0) + q * N, np.full(l1, slot + q * N)]
            Rl += [rel(l0, r0), rel(l1, r1)]
            T += [np.full(l0, slot + q * N), other(l1) + q * N]
            placed.append((q, slot, l0, l1))
        n = int(spec.get("extra", 0))
        if n:
            i = np.arange(n)
            H.append(sinks[i % len(sinks)] + q * N)
            Rl.append(rel(n))
            T.append(sinks[(5 * i + 3 + i // len(sinks)) % len(sinks)] + q * N)
    if H:
        h, r, t = (np.concatenate(x).astype(np.int64) for x in (H, Rl, T))
    else:
        h = r = t = np.zeros(0, np.int64)
    p = rng.permutation(len(h))
    return Graph(name, B, N, R, h[p], r[p], t[p], placed)


# ---- the graphs of the case table -------------------------------------------------------------------------------

_CACHE = {}


def graph(name):
    if name not in _CACHE:
        _CACHE[name] = GRAPHS[name]()
    return _CACHE[name]


def _light_places():
    return [(l, 0) for l in LIGHT_LADDER[1:]] + [(0, l) for l in LIGHT_LADDER[1:]] + list(MERGED_PAIRS) + [(0, 0)]


def _medium_places():
    out = []
    for i, l in enumerate(MEDIUM_LADDER):
        out += [(l, i % 2), (i % 2, l)]                        # the other direction 0 or 1
    return out + [(33, 33), (64, 513), (512, 65), (4095, 1), (2048, 2049), (4096, 4096), (65, 0), (0, 129)]


def _huge_places():
    a, b = HUGE_LADDER
    return [(a, 0), (b, 0), (0, a), (0, b), (a, a), (b, b)]


def g_ladder(R=400, name="ladder"):
    """B = 3, N = 203 (13 sets, the last of 11 nodes).  Question 0: the light ladder in each direction and the merged
    runs, 5 relations.  Question 1: medium rows, every relation, 40 sinks so that the big-node list stays below its
    cap (26 placed + 40).  Question 2: huge rows, 17 relations."""
    return build_graph(name, 3, 203, R, [
        dict(place=_light_places(), nrel=5, extra=300),
        dict(place=_medium_places(), nrel=None, sinks=40, extra=R),
        dict(place=_huge_places(), nrel=17, sinks=30)], seed=11)


def g_bigcap():
    """Question 0: exactly 72 big nodes (33 facts arriving, sources spread over 131 light sinks), question 1: 73 (the
    walk then has no list: lane groups walk the 33-fact rows), question 2: no facts."""
    g = build_graph("bigcap", 3, 203, 40, [
        dict(place=[(33, i % 3) for i in range(72)], nrel=16),
        dict(place=[(33, i % 3) for i in range(72)] + [(1, 40)], nrel=17),
        None], seed=12)
    assert len(g.big_nodes(0)) == BIG_CAP and len(g.big_nodes(1)) == BIG_CAP + 1 and g.len0[2 * 203:].sum() == 0
    return g


def g_relcounts():
    """Seven small questions that use 1, 3, 4, 5, 16, 17 and every one of 40 relations; N = 45."""
    lad = [(l, 0) for l in (1, 3, 4, 5, 7, 8, 9)] + [(0, l) for l in (1, 4, 5, 8, 9, 12)] + [(8, 1), (8, 8), (16, 1), (17, 16)]
    return build_graph("relcounts", 7, 45, 40, [dict(place=lad, nrel=k, extra=60) for k in (1, 3, 4, 5, 16, 17, None)],
                       seed=13)


def _tiny_questions(name, B, N, R, seed, special=None):
    """B small questions with a few ladder rows each; question 0 uses every one of the R relations (R > 301 selects the
    16-column slices); ``special`` = {question: places} replaces a question's rows."""
    lad = list(LIGHT_LADDER[1:]) + [8, 16]
    qs = []
    for q in range(B):
        place = [(lad[(q + 3 * i) % len(lad)], i % 2) if i % 3 else (i % 2, lad[(q + 5 * i) % len(lad)]) for i in range(9)]
        spec = dict(place=place, nrel=(None if q == 0 else 1 + (q % 17)), extra=(R if q == 0 else 20))
        if special and q in special:
            spec = dict(place=special[q], nrel=5, extra=20)
        qs.append(spec)
    return build_graph(name, B, N, R, qs, seed=seed)


def g_b41():
    """B = 41, N = 43: 6 x 13 = 78 items per XCD against 64 (76) slots - full rounds plus a split tail.  Question 40 is
    alone in the last group, all (at 304 CUs: the last two) of its slices are cut in two: it holds two huge rows, a
    medium one and light sets on both sides of the cut."""
    return _tiny_questions("b41", 41, 43, 320, 14, {40: [(4097, 0), (0, 4100), (513, 1), (65, 64), (9, 8), (5, 0), (0, 17)]})


def g_b57():
    return _tiny_questions("b57", 57, 43, 320, 15)


def g_b32():
    return _tiny_questions("b32", 32, 43, 320, 16)


def g_b1_n1024():
    """B = 1, N = 1028 (65 sets, the last of 4 nodes): every item cut into four node ranges (pl = 2); four huge rows so
    that every range owns one, medium rows, the light ladder."""
    place = [(4097, 0), (0, 4097), (4200, 1), (1, 4300), (513, 0), (0, 64), (65, 33), (4096, 0)] + _light_places()
    return build_graph("b1_n1024", 1, 1028, 320, [dict(place=place, nrel=None, sinks=60, extra=2000)], seed=17)


def g_b1_n2048():
    """B = 1, N = 2051: pl = 3, eight node ranges."""
    place = [(4097, 0), (0, 4097)] + [(33 + i, i % 2) for i in range(9)] + _light_places()
    return build_graph("b1_n2048", 1, 2051, 30, [dict(place=place, nrel=None, sinks=60, extra=4000)], seed=18)


def g_hubs(R=1300, counts=(1, 16, 17, 33, 49), name="hubs", extra=6000):
    """Gather walk (a question uses all R > 1235 relations: the tables outgrow LDS): questions with 1, 16, 17, 33 and 49
    hubs (rows of more than 256 facts in a direction; hub tiles of 16 / 32 / 48), hub sizes 257 .. 300 and a few of
    512 / 513, alternating directions; question 0's hub holds ONE relation over 13 chunks; the 16-hub question holds a hub
    of 257 facts with 257 relations, one whose first relation run is exactly 256 facts (it ends on a chunk boundary)
    and one of exactly 256 facts (not a hub); relation counts 1300, 3, 4, 5, 16 / 17 of them so that nrel is no multiple
    of 4 or 16; a last question without hubs."""
    qs = []
    for qi, c in enumerate(counts):
        place = []
        for i in range(c):
            n = (257, 258, 263, 300, 512, 513, 271, 289)[i % 8]
            place.append((n, 0) if (i + qi) % 2 else (0, n))
        nrel = (None, 3, 17, 5, 16)[qi % 5]
        if qi == 0:
            place[0] = (0, 3300, None, np.full(3300, 7))
        if c >= 16:
            place[1] = (0, 257, None, np.arange(300, 557))
            place[2] = (600, 0, np.r_[np.full(256, 2), np.arange(600, 600 + 344)], None)
            place.append((256, 1))
        qs.append(dict(place=place, nrel=nrel, extra=(R + 200 if nrel is None else extra)))
    qs.append(dict(place=[(l, 0) for l in (1, 4, 5, 64, 65, 128, 129, 255, 256)], nrel=4, extra=200))
    g = build_graph(name, len(qs), 301, R, qs, seed=19)
    per_q = np.bincount(np.r_[g.hubs(0), g.hubs(1)] // g.N, minlength=g.B)
    assert per_q.tolist() == list(counts) + [0], per_q
    return g


def g_hubs_small():
    return g_hubs(counts=(1, 17), name="hubs_small", extra=6000)


def g_hub_blocks():
    """90 hubs of 260 facts per question over all 1300 relations: the hub-by-relation weight blocks and partial rows
    outgrow their workspace region (16 B per fact) - the device-side decision must be the chunked fallback."""
    q = dict(place=[(0, 260) for _ in range(90)], nrel=None, extra=1300)
    return build_graph("hub_blocks", 2, 301, 1300, [q, q], seed=20)


def g_frontier_hub():
    """One row of 4097 facts (kWfAltMin = 4096) whose sources are 202 nodes with about 20 facts each."""
    return build_graph("frontier_hub", 2, 203, 40, [dict(place=[(4097, 0)], nrel=16, extra=100),
                                                    dict(place=[(0, 4097), (5, 3)], nrel=5, extra=100)], seed=21)


def g_frontier_wide():
    """N = 2100 > 2048: a question can hold more seeds than the LDS seed list."""
    return build_graph("frontier_wide", 2, 2100, 40, [dict(place=_light_places(), nrel=16, extra=5000),
                                                      dict(place=_light_places(), nrel=5, extra=3000)], seed=22)


GRAPHS = {"ladder": g_ladder, "ladder32": lambda: g_ladder(60, "ladder32"), "bigcap": g_bigcap, "relcounts": g_relcounts,
          "b41": g_b41, "b57": g_b57, "b32": g_b32, "b1_n1024": g_b1_n1024, "b1_n2048": g_b1_n2048, "hubs": g_hubs,
          "hubs_small": g_hubs_small, "hub_blocks": g_hub_blocks, "frontier_hub": g_frontier_hub,
          "frontier_wide": g_frontier_wide}


# ---- exact data families ------------------------------------------------------------------------------------------

def exact_priors(g, rng):
    """m 2^-10, m in [0, 15]: 40 % zeros, 20 % non-zero only in the low range (m <= 3)."""
    m = rng.integers(1, 16, g.B * g.N)
    u = rng.random(g.B * g.N)
    m[u < 0.4] = 0
    low = (u >= 0.4) & (u < 0.6)
    m[low] = rng.integers(1, 4, int(low.sum()))
    return (m * 2.0 ** -10).astype(np.float32).reshape(g.B, g.N)


def exact_weights(g, rng):
    return rng.choice(np.array([0.5, 1.0, 2.0], np.float32), g.F)


def exact_ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, shape).astype(np.float32)


def random_priors(g, rng):
    """softmax of 6 standard_normal per question: about eight decades."""
    z = 6.0 * rng.standard_normal((g.B, g.N))
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def certify(what, factors, bound, want):
    """``factors`` = [(array, unit)]: every entry a multiple of its unit; u = product of the units; ``bound`` >= the
    sum of |terms| of every output entry; ``want`` (float64) equals its fp32 rounding.  Returns u."""
    u = 1.0
    for a, unit in factors:
        x = np.asarray(a, np.float64) / unit
        assert np.array_equal(x, np.round(x)), what + ": a factor is off its grid"
        u *= unit
    assert float(np.max(bound, initial=0.0)) < 2.0 ** 24 * u, (what, float(np.max(bound)), 2.0 ** 24 * u)
    x = np.asarray(want) / u
    assert np.array_equal(x, np.round(x)), what + ": result off the grid"
    assert np.array_equal(np.asarray(want), np.asarray(want).astype(np.float32).astype(np.float64)), what
    return u


# ---- float64 references from the caller's tuple ---------------------------------------------------------------------

def _scatter(idx, vals, n):
    """out[i] = sum of vals[j] over idx[j] == i (float64)."""
    vals = np.asarray(vals, np.float64)
    out = np.zeros((n,) + vals.shape[1:])
    if len(idx) == 0:
        return out
    o = np.argsort(idx, kind="stable")
    si = idx[o]
    starts = np.flatnonzero(np.r_[True, si[1:] != si[:-1]])
    out[si[starts]] = np.add.reduceat(vals[o], starts, axis=0)
    return out


def _coef_blocks(g, coef, dst, col, ncols):
    """Per question b: C [N, ncols[b]] with C[dst - b N, col] = sum of coef over the question's facts - a fact's term is
    coef x (a table row that depends on (question, col) only), so a walk's sum is C @ table."""
    for b in range(g.B):
        i = g.q_order[g.q_ptr[b]:g.q_ptr[b + 1]]
        nc = int(ncols[b])
        yield b, np.bincount((dst[i] - b * g.N) * nc + col[i], weights=coef[i], minlength=g.N * nc).reshape(g.N, nc)


def _w2(g, w):
    return np.ones(g.F) if w is None else np.asarray(w, np.float64) ** 2


def _dirs(g):
    """(direction, source node, destination node) of every fact, per direction."""
    return ((0, g.h, g.t), (1, g.t, g.h))


def ref_fused(g, dist, P, w=None, dirs=(0, 1), absolute=False):
    """out[dst] = sum_f w_f^2 dist[src_f] P[d][row(question, rel_f)]  (reasongnn.py:80-116, factored form)."""
    f = np.abs if absolute else (lambda x: x)
    d64, P64, w2 = f(np.asarray(dist, np.float64).reshape(-1)), f(np.asarray(P, np.float64)), _w2(g, w)
    out = np.zeros((g.B * g.N, P64.shape[-1]))
    col = g.row_of - g.rel_off[g.h // g.N]                      # the relation's row inside its question's tables
    for d, src, dst in _dirs(g):
        if d in dirs:
            for b, C in _coef_blocks(g, w2 * d64[src], dst, col, g.rel_cnt):
                out[b * g.N:(b + 1) * g.N] += C @ P64[d][g.rel_off[b]:g.rel_off[b + 1]]
    return out


def ref_row_terms(g):
    """Number of facts of every row (both directions) and relations of its question: n and k of the per-row bound."""
    return g.len0 + g.len1, np.repeat(g.rel_cnt, g.N)


def ref_unfused(g, dist, ins, Tf, Ti, w=None, absolute=False):
    """agg [BN, 2 I D]: blocks (i, forward), (i, inverse) of w^2 dist[src] relu(T_d[rel] * ins[question, i])."""
    f = np.abs if absolute else (lambda x: x)
    d64, w2 = np.asarray(dist, np.float64).reshape(-1), _w2(g, w)
    ins64 = np.asarray(ins, np.float64)
    B, I, D = ins64.shape
    out = np.zeros((g.B * g.N, 2 * I * D))
    for (d, src, dst), T in zip(_dirs(g), (Tf, Ti)):
        T64 = np.asarray(T, np.float64)
        for b, C in _coef_blocks(g, w2 * d64[src], dst, g.r, np.full(g.B, g.R)):
            for i in range(I):                                      # (terms are >= 0: f changes nothing, kept for symmetry)
                out[b * g.N:(b + 1) * g.N, (2 * i + d) * D:(2 * i + d + 1) * D] = C @ f(np.maximum(T64 * ins64[b, i], 0.0))
    return out


def ref_typelayer(g, T, wrel=None, absolute=False):
    """relu(sum over incident facts, tail side + head side, of v_f T[rel_f]); ``absolute``: the sum of |terms|."""
    f = np.abs if absolute else (lambda x: x)
    v = np.ones(g.F) if wrel is None else np.asarray(wrel, np.float64)
    val = f(v[:, None] * np.asarray(T, np.float64)[g.r])
    pre = _scatter(g.t, val, g.B * g.N) + _scatter(g.h, val, g.B * g.N)
    return pre if absolute else np.maximum(pre, 0.0)           # the walk applies TypeLayer's ReLU (layer_init.py:25-62)


def ref_frontier(g, dist, P, w=None):
    """(row gates, out): node n is listed iff a fact arrives at it from a node with dist != 0; out = the fused walk."""
    nz = np.asarray(dist).reshape(-1) != 0
    flag = np.zeros(g.B * g.N, bool)
    flag[g.t[nz[g.h]]] = True
    flag[g.h[nz[g.t]]] = True
    return flag, ref_fused(g, dist, P, w)


def ref_fused_backward(g, dist, P, gn, w=None, absolute=False):
    """g_dist [BN], g_P [2, rel_total, D] of ref_fused for the upstream gradient gn [BN, D]."""
    f = np.abs if absolute else (lambda x: x)
    d64, P64, g64, w2 = (f(np.asarray(dist, np.float64).reshape(-1)), f(np.asarray(P, np.float64)),
                         f(np.asarray(gn, np.float64)), _w2(g, w))
    gd = np.zeros(g.B * g.N)
    gP = np.zeros_like(P64)
    for d, src, dst in _dirs(g):
        gd += _scatter(src, w2 * np.einsum("fd,fd->f", g64[dst], P64[d][g.row_of]), g.B * g.N)
        gP[d] = _scatter(g.row_of, (w2 * d64[src])[:, None] * g64[dst], g.rel_total)
    return gd, gP


def ref_unfused_backward(g, dist, ins, Tf, Ti, gagg, w=None, absolute=False):
    """g_dist [BN], g_ins [B, I, D], g_T_fwd, g_T_inv [R, D] of ref_unfused; the ReLU passes where T * ins > 0."""
    f = np.abs if absolute else (lambda x: x)
    d64, w2 = np.asarray(dist, np.float64).reshape(-1), _w2(g, w)
    ins64, ga = np.asarray(ins, np.float64), np.asarray(gagg, np.float64)
    B, I, D = ins64.shape
    q = g.h // g.N
    gd, gi, gT = np.zeros(g.B * g.N), np.zeros_like(ins64), [np.zeros((g.R, D)), np.zeros((g.R, D))]
    for i in range(I):
        for (d, src, dst), T in zip(_dirs(g), (Tf, Ti)):
            Tr = np.asarray(T, np.float64)[g.r]
            gate = (Tr * ins64[q, i]) > 0
            gb = ga[dst, (2 * i + d) * D:(2 * i + d + 1) * D] * gate
            gd += _scatter(src, w2 * f(gb * Tr * ins64[q, i]).sum(1), g.B * g.N)
            wp = (w2 * d64[src])[:, None]
            gi[:, i] += _scatter(q, f(wp * gb * Tr), B)
            gT[d] += _scatter(g.r, f(wp * gb * ins64[q, i]), g.R)
    return gd, gi, gT[0], gT[1]


def ref_typelayer_backward(g, gpre, wrel=None, absolute=False):
    f = np.abs if absolute else (lambda x: x)
    v = np.ones(g.F) if wrel is None else np.asarray(wrel, np.float64)
    g64 = np.asarray(gpre, np.float64)
    return _scatter(g.r, f(v[:, None] * g64[g.t]) + f(v[:, None] * g64[g.h]), g.R)


def f32_stored_order(g, dist, P, w=None):
    """The yardstick of the 8x rule: numpy float32 sum of the same terms, one after the other in stored order (a row's
    direction-0 facts in fact order, then its direction-1 facts)."""
    d32 = np.asarray(dist, np.float32).reshape(-1)
    out = np.zeros((g.B * g.N, P.shape[-1]), np.float32)
    for d, src, dst in _dirs(g):
        p = d32[src] if w is None else d32[src] * (np.asarray(w, np.float32) ** 2)
        np.add.at(out, dst, p[:, None] * np.asarray(P, np.float32)[d][g.row_of])
    return out


def _f32(*a):
    return [np.asarray(x, np.float32) for x in a]


def _pw32(g, dist, w, src):
    p = np.asarray(dist, np.float32).reshape(-1)[src]
    return p if w is None else p * (np.asarray(w, np.float32) ** 2)


def f32_stored_order_unfused(g, dist, ins, Tf, Ti, w=None):
    ins32, q = np.asarray(ins, np.float32), g.h // g.N
    blocks = []
    for i in range(ins32.shape[1]):
        for (d, src, dst), T in zip(_dirs(g), (Tf, Ti)):
            out = np.zeros((g.B * g.N, ins32.shape[2]), np.float32)
            np.add.at(out, dst, _pw32(g, dist, w, src)[:, None] * np.maximum(np.asarray(T, np.float32)[g.r] * ins32[q, i], 0))
            blocks.append(out)
    return np.concatenate(blocks, axis=1)


def f32_stored_order_typelayer(g, T, wrel=None):
    v = np.ones(g.F, np.float32) if wrel is None else np.asarray(wrel, np.float32)
    val = v[:, None] * np.asarray(T, np.float32)[g.r]
    out = np.zeros((g.B * g.N, val.shape[1]), np.float32)
    np.add.at(out, g.t, val)
    np.add.at(out, g.h, val)
    return np.maximum(out, 0)


def f32_fused_backward(g, dist, P, gn, w=None):
    """float32 yardstick of the fused backward: per-fact dot products in float32, added one after the other."""
    P32, g32 = _f32(P, gn)
    gd, gP = np.zeros(g.B * g.N, np.float32), np.zeros_like(P32)
    w2 = np.ones(g.F, np.float32) if w is None else np.asarray(w, np.float32) ** 2
    for d, src, dst in _dirs(g):
        np.add.at(gd, src, w2 * np.cumsum(g32[dst] * P32[d][g.row_of], axis=1, dtype=np.float32)[:, -1])
        np.add.at(gP[d], g.row_of, _pw32(g, dist, w, src)[:, None] * g32[dst])
    return gd, gP


def f32_unfused_backward(g, dist, ins, Tf, Ti, gagg, w=None):
    ins32, ga = _f32(ins, gagg)
    B, I, D = ins32.shape
    q = g.h // g.N
    w2 = np.ones(g.F, np.float32) if w is None else np.asarray(w, np.float32) ** 2
    gd, gi = np.zeros(g.B * g.N, np.float32), np.zeros_like(ins32)
    gT = [np.zeros((g.R, D), np.float32), np.zeros((g.R, D), np.float32)]
    for i in range(I):
        for (d, src, dst), T in zip(_dirs(g), (Tf, Ti)):
            Tr = np.asarray(T, np.float32)[g.r]
            gb = ga[dst, (2 * i + d) * D:(2 * i + d + 1) * D] * ((Tr * ins32[q, i]) > 0)
            np.add.at(gd, src, w2 * np.cumsum(gb * Tr * ins32[q, i], axis=1, dtype=np.float32)[:, -1])
            wp_ = _pw32(g, dist, w, src)[:, None]
            np.add.at(gi[:, i], q, wp_ * gb * Tr)
            np.add.at(gT[d], g.r, wp_ * gb * ins32[q, i])
    return gd, gi, gT[0], gT[1]


def f32_typelayer_backward(g, gpre, wrel=None):
    v = np.ones(g.F, np.float32) if wrel is None else np.asarray(wrel, np.float32)
    g32 = np.asarray(gpre, np.float32)
    out = np.zeros((g.R, g32.shape[1]), np.float32)
    np.add.at(out, g.r, v[:, None] * g32[g.t])
    np.add.at(out, g.r, v[:, None] * g32[g.h])
    return out


# ---- the host-side launch arithmetic, restated ------------------------------------------------------------------------

def _slice_lds_bytes(rows, na, width):
    return 2 * (rows + 1) * width * 4 + (16 + 5 * BIG_CAP) * 4 + na * 16 * 16 * 4


def walk_variant(rel_max, D):
    """gnnrag_aggregate_fused_variant."""
    if D % 4 or _slice_lds_bytes(rel_max, 3, 16) > 160 * 1024 - 1024:
        return WALK_L2_GATHER
    if D > 16 and _slice_lds_bytes(rel_max, 2, 32) <= 79 * 1024:
        return WALK_LDS_32
    return WALK_LDS_16


def launch_regime(B, N, D, variant, cus):
    """pl / nfull of launch_slice (csrc/aggregate.hip) and the name of the regime."""
    sw = 32 if variant == WALK_LDS_32 else 16
    nslice = (D + sw - 1) // sw
    slots = 2 * (cus // 8) if cus >= 8 else 2
    items = ((B + 7) // 8) * nslice
    rem = items % slots
    nfull = items - rem if rem else items
    pl = 0
    if B <= 8:
        while pl < 3 and (items << (pl + 1)) <= slots and ((N // 16) >> (pl + 1)) >= 16:
            pl += 1
        if pl < 2:
            pl = 0
    if pl:
        name = "pl=%d" % pl
    elif nfull == items:
        name = "no split"
    elif nfull == 0:
        name = "every item split"
    else:
        name = "full rounds plus a split tail"
    return dict(nslice=nslice, sw=sw, slots=slots, items=items, nfull=nfull, pl=pl, regime=name)


def item_parts(reg, q, c):
    """Into how many node ranges the item (question q, slice c) is cut."""
    if reg["pl"]:
        return 1 << reg["pl"]
    item = (q // 8) * reg["nslice"] + c
    return 2 if item >= reg["nfull"] else 1


def hub_form(g, D, enabled=True):
    """prepare_fused + hub_dense_on: which form the hub rows of a gather-walk call take."""
    if walk_variant(g.rel_max, D) != WALK_L2_GATHER or D % 4 or D > 256 or not enabled or g.R <= 1024:
        return HUB_FORM_NONE
    heavy_cap = max(g.F, 1) // HEAVY_DEG + 1
    avail = -(-2 * max(g.F, 1) * 8 // 256) * 256
    bnd = -(-2 * 2 * heavy_cap * 8 // 256) * 256
    if avail <= bnd + 4096:
        return HUB_FORM_NONE
    cap = min((avail - bnd) // 4, 1 << 30)
    ks = min(max((64 * HUB_KS_MAX) // (2 * g.B), 1), HUB_KS_MAX)
    nrel4 = (g.rel_cnt + 3) & ~3
    hubs = [np.bincount(g.hubs(d) // g.N, minlength=g.B) for d in (0, 1)]
    total = sum(int((hd * nrel4).sum()) for hd in hubs)
    nh = sum(int(hd.sum()) for hd in hubs)
    return HUB_FORM_DENSE if total + nh * ks * D <= cap else HUB_FORM_CHUNKED


# ---- the walk's structure as a numpy model, with a flaw --------------------------------------------------------------

FLAWS = ("drop_last_mod4", "drop_last_mod8", "drop_last_mod64", "second_from_dir0", "drop_last_float4",
         "skip_small_prior", "skip_partial_last_set", "huge_missing_in_one_part", "skip_last_question",
         "hub_run_twice", "weight_unsquared", "swap_tables")


def _model_rows(g, q, nl, coef, tab, row, P64):
    """Rows of question q: sum over its records of coef x P[tab][row], as (N x 2 Rq coefficients) @ (both tables)."""
    ro, Rq = int(g.rel_off[q]), int(g.rel_cnt[q])
    if Rq == 0:
        return np.zeros((g.N, P64.shape[-1]))
    C = np.bincount(nl * (2 * Rq) + tab * Rq + (row - ro), weights=coef, minlength=g.N * 2 * Rq).reshape(g.N, 2 * Rq)
    return C @ np.concatenate([P64[0][ro:ro + Rq], P64[1][ro:ro + Rq]])


def walk_model(g, dist, P, w=None, flaw=None, cus=256):
    """The fused walk of (g, dist, P, w) as the kernels organise it, in float64 - with ``flaw`` one deliberate mistake:

    drop_last_mod4 / mod8   a lane-group row (4 facts per quad step, 8 per step) loses its last fact when len % 4 (8) == 1
    drop_last_mod64         a wave-walked row (medium, huge) loses its last fact when len % 64 == 1
    second_from_dir0        records 8..15 of a light merged run are taken from direction 0's run only
    drop_last_float4        the last float4 of the last column slice is not written
    skip_small_prior        facts whose prior is below 2^-7 of the row's largest are skipped
    skip_partial_last_set   the nodes of the last, partial 16-node set are not walked by the lane groups
    huge_missing_in_one_part  in an item cut into parts, the huge nodes of the last part are not walked
    skip_last_question      question B - 1 is not walked when B % 8 != 0
    hub_run_twice           gather walk: a hub's relation run that ends on a 256-fact chunk boundary is added twice
    weight_unsquared        the per-fact weight enters once
    swap_tables             direction 0 reads direction 1's table and the other way round
    """
    assert flaw is None or flaw in FLAWS, flaw
    B, N, BN = g.B, g.N, g.B * g.N
    P64 = np.asarray(P, np.float64)
    D = P64.shape[-1]
    d64 = np.asarray(dist, np.float64).reshape(-1)
    weff = np.ones(g.F) if w is None else np.asarray(w, np.float64) ** (1 if flaw == "weight_unsquared" else 2)
    # the merged record stream: a node's direction-0 facts in fact order, then its direction-1 facts
    dst = np.r_[g.t, g.h]
    src = np.r_[g.h, g.t]
    tab = np.r_[np.zeros(g.F, np.int64), np.ones(g.F, np.int64)]
    fid = np.r_[np.arange(g.F), np.arange(g.F)]
    o = np.argsort(dst * 2 + tab, kind="stable")
    dst, src, tab, fid = dst[o], src[o], tab[o], fid[o]
    rp = np.searchsorted(dst, np.arange(BN + 1))
    pw = weff[fid] * d64[src]
    row = g.row_of[fid]
    rel = g.r[fid]
    tabr = 1 - tab if flaw == "swap_tables" else tab
    variant = walk_variant(g.rel_max, D)
    out = np.zeros((BN, D))
    if variant == WALK_L2_GATHER:
        keep = np.ones(len(dst))
        if flaw == "hub_run_twice":
            for d, lens in ((0, g.len0), (1, g.len1)):
                for n in np.flatnonzero(lens > HEAVY_DEG):
                    b = rp[n] + (g.len0[n] if d else 0)
                    e = b + lens[n]
                    ro = np.argsort(rel[b:e], kind="stable")           # hub rows are stored in relation order
                    rs = rel[b:e][ro]
                    ends = np.flatnonzero(np.r_[rs[1:] != rs[:-1], True]) + 1
                    begs = np.r_[0, ends[:-1]]
                    for rb, re_ in zip(begs, ends):
                        if re_ % HEAVY_DEG == 0 and re_ < lens[n]:
                            keep[b + ro[rb:re_]] = 2.0
        for q in range(B):
            lo, hi = rp[q * N], rp[(q + 1) * N]
            out[q * N:(q + 1) * N] = _model_rows(g, q, dst[lo:hi] - q * N, (keep * pw)[lo:hi], tabr[lo:hi], row[lo:hi], P64)
        return out
    for q in range(B):
        if flaw == "skip_last_question" and B % 8 and q == B - 1:
            continue
        reg = launch_regime(B, N, D, variant, cus)
        nodes = np.arange(q * N, (q + 1) * N)
        l0, l1 = g.len0[nodes], g.len1[nodes]
        ln = l0 + l1                                               # the merged run
        big = np.maximum(l0, l1) > BIG_DEG
        blist = np.flatnonzero(big)
        listed = big if len(blist) <= BIG_CAP else np.zeros(N, bool)
        wave_row = listed                                          # medium and huge: 64 facts per step
        huge = listed & (ln > TEAM_DEG)
        lo, hi = rp[q * N], rp[(q + 1) * N]
        j = np.arange(lo, hi) - rp[dst[lo:hi]]                      # position of a record in its run
        nl = dst[lo:hi] - q * N
        keep = np.ones(hi - lo)
        last = j == ln[nl] - 1
        if flaw == "drop_last_mod4":
            keep[last & ~wave_row[nl] & (ln[nl] % 4 == 1)] = 0
        if flaw == "drop_last_mod8":
            keep[last & ~wave_row[nl] & (ln[nl] % 8 == 1)] = 0
        if flaw == "drop_last_mod64":
            keep[last & wave_row[nl] & (ln[nl] % 64 == 1)] = 0
        if flaw == "second_from_dir0":
            keep[~wave_row[nl] & (j >= 8) & (j < 16) & (j >= l0[nl])] = 0
        if flaw == "skip_small_prior":
            mx = np.zeros(N)
            np.maximum.at(mx, nl, pw[lo:hi])
            keep[pw[lo:hi] < mx[nl] * 2.0 ** -7] = 0
        full = _model_rows(g, q, nl, keep * pw[lo:hi], tabr[lo:hi], row[lo:hi], P64)
        covered = np.zeros((N, reg["nslice"]), np.int64)
        for c in range(reg["nslice"]):
            c0, c1 = c * reg["sw"], min(D, (c + 1) * reg["sw"])
            if flaw == "drop_last_float4" and c == reg["nslice"] - 1:
                c1 -= 4
            nparts = item_parts(reg, q, c)
            for part in range(nparts):
                walk = np.zeros(N, bool)
                bl = blist if listed.any() else blist[:0]
                mine = bl[np.arange(len(bl)) % nparts == part]     # the big-node list: entry h belongs to part h % nparts
                if flaw == "huge_missing_in_one_part" and nparts > 1 and part == nparts - 1:
                    mine = mine[~huge[mine]]
                walk[mine] = True
                sets = np.arange(part, (N + 15) // 16, nparts)     # light sets part, part + nparts, ...
                for s in sets:
                    if flaw == "skip_partial_last_set" and N % 16 and s == (N + 15) // 16 - 1:
                        continue
                    m = np.arange(16 * s, min(16 * s + 16, N))
                    walk[m[~listed[m]]] = True
                covered[walk, c] += 1
                out[np.ix_(nodes[walk], np.arange(c0, c1))] = full[np.ix_(walk, np.arange(c0, c1))]
        if flaw is None:
            assert (covered == 1).all(), (g.name, q)
    return out


# ---- the case table of tests/test_gpu_walks_exact.py -----------------------------------------------------------------
# fused cases: (name, graph, D, variant the case means to test, regime at 256 CUs or None, hub form or None)

FUSED_CASES = [
    ("ladder_d200", "ladder", 200, WALK_LDS_16, "every item split", None),
    ("ladder_d16", "ladder", 16, WALK_LDS_16, "every item split", None),
    ("ladder_d20", "ladder", 20, WALK_LDS_16, "every item split", None),
    ("ladder_d4", "ladder", 4, WALK_LDS_16, "every item split", None),
    ("ladder32_d200", "ladder32", 200, WALK_LDS_32, "every item split", None),
    ("ladder32_d72", "ladder32", 72, WALK_LDS_32, "every item split", None),
    ("relcounts_d200", "relcounts", 200, WALK_LDS_32, "every item split", None),
    ("relcounts_d64", "relcounts", 64, WALK_LDS_32, "every item split", None),
    ("relcounts_d36", "relcounts", 36, WALK_LDS_32, "every item split", None),
    ("bigcap_d20", "bigcap", 20, WALK_LDS_32, "every item split", None),
    ("bigcap_d16", "bigcap", 16, WALK_LDS_16, "every item split", None),
    ("b41_d200", "b41", 200, WALK_LDS_16, "full rounds plus a split tail", None),
    ("b57_d128", "b57", 128, WALK_LDS_16, "no split", None),
    ("b32_d304", "b32", 304, WALK_LDS_16, "full rounds plus a split tail", None),      # 304 CUs: no split
    ("b1_n1024_d200", "b1_n1024", 200, WALK_LDS_16, "pl=2", None),
    ("b1_n2048_d16", "b1_n2048", 16, WALK_LDS_16, "pl=3", None),
    ("hubs_d200", "hubs", 200, WALK_L2_GATHER, None, HUB_FORM_DENSE),
    ("hubs_small_d132", "hubs_small", 132, WALK_L2_GATHER, None, HUB_FORM_DENSE),
    ("hubs_small_d256", "hubs_small", 256, WALK_L2_GATHER, None, HUB_FORM_DENSE),
    ("hub_blocks_d200", "hub_blocks", 200, WALK_L2_GATHER, None, HUB_FORM_CHUNKED),
    ("ladder32_d30", "ladder32", 30, WALK_L2_GATHER, None, HUB_FORM_NONE),             # D % 4 != 0 at a small R
]
FUSED_BY_NAME = {c[0]: c for c in FUSED_CASES}
UNFUSED_CASES = [(1, 50), (2, 200), (3, 50), (4, 200)]            # (I, D) on ladder32; I = 4: second launch of the i0 loop
FRONTIER_CASES = ("one_seed", "reaches_4097_row", "more_seeds_than_the_list", "sentinel")
BACKWARD_CASES = [("ladder32", 20), ("hubs_small", 64)]           # (graph, D)
# What the GPU file runs: the LDS-walk cases and the backward on the ladder graph.  The gather-walk cases and the hub
# graphs (more than 1024 relations) are host-only fixtures for now ("What pins the walks").
GPU_FUSED_CASES = [c[0] for c in FUSED_CASES if c[3] != WALK_L2_GATHER]
GPU_BACKWARD_CASES = BACKWARD_CASES[:1]
# the launch regime every LDS-walk case is meant to reach, per CU count (FUSED_CASES states it for 256 CUs; at 304 the
# slots per XCD are 76 instead of 64, which moves two cases)
REGIME_AT = {256: {c[0]: c[4] for c in FUSED_CASES if c[3] != WALK_L2_GATHER}}
REGIME_AT[304] = dict(REGIME_AT[256], b57_d128="every item split", b32_d304="no split")


def fused_data(name, weights, exact=True):
    """(graph, dist, P, w) of a fused case: the arrays that go to the device."""
    _, gname, D, _, _, _ = FUSED_BY_NAME[name]
    g = graph(gname)
    rng = np.random.default_rng(sum(map(ord, name)) * 4 + 2 * bool(weights) + bool(exact))
    if exact:
        dist = exact_priors(g, rng)
        P = exact_ints(rng, (2, g.rel_total, D), 4)
        w = exact_weights(g, rng) if weights else None
    else:
        dist = random_priors(g, rng)
        P = rng.standard_normal((2, g.rel_total, D)).astype(np.float32)
        w = (0.5 + rng.random(g.F)).astype(np.float32) if weights else None
    return g, dist, P, w


def certify_fused(what, g, dist, P, w, want):
    """The certificate of a fused case; the bound sum_f w^2 p max|P| covers every column of the row."""
    w2p = _w2(g, w)
    bound = (_scatter(g.t, w2p * np.asarray(dist, np.float64).reshape(-1)[g.h], g.B * g.N)
             + _scatter(g.h, w2p * np.asarray(dist, np.float64).reshape(-1)[g.t], g.B * g.N)) * float(np.abs(P).max(initial=0))
    fac = [(dist, 2.0 ** -10), (P, 1.0)] + ([(np.asarray(w, np.float64) ** 2, 0.25)] if w is not None else [])
    return certify(what, fac, bound, want)


def certify_unfused(g, dist, ins, Tf, Ti, w, want):
    """Bound: sum_f w^2 p max|T| max|ins| covers every column of every block of the row."""
    d64 = np.asarray(dist, np.float64).reshape(-1)
    bound = ((_scatter(g.t, _w2(g, w) * d64[g.h], g.B * g.N) + _scatter(g.h, _w2(g, w) * d64[g.t], g.B * g.N))
             * float(max(np.abs(Tf).max(), np.abs(Ti).max()) * np.abs(ins).max()))
    fac = [(dist, 2.0 ** -10), (Tf, 1.0), (Ti, 1.0), (ins, 1.0)] + ([(np.asarray(w, np.float64) ** 2, 0.25)] if w is not None else [])
    return certify("unfused", fac, bound, want)


def certify_typelayer(g, T, w, want):
    return certify("typelayer", [(T, 1.0)] + ([(w, 0.5)] if w is not None else []), ref_typelayer(g, T, w, absolute=True), want)


def certify_backward(g, d):
    """The certificates of every gradient of a backward case; returns the float64 references
    ((g_dist, g_P), (g_dist, g_ins, g_T_fwd, g_T_inv), {with w_rel: g_T})."""
    w2 = (np.asarray(d["w"], np.float64) ** 2, 0.25)
    p, one = (d["dist"], 2.0 ** -10), lambda a: (a, 1.0)
    fused = ref_fused_backward(g, d["dist"], d["P"], d["gn"], d["w"])
    a = ref_fused_backward(g, d["dist"], d["P"], d["gn"], d["w"], absolute=True)
    certify("fused g_dist", [w2, one(d["P"]), one(d["gn"])], a[0], fused[0])
    certify("fused g_P", [w2, p, one(d["gn"])], a[1], fused[1])
    r = ref_unfused_backward(g, d["dist"], d["ins"], d["Tf"], d["Ti"], d["gagg"], d["w"])
    a = ref_unfused_backward(g, d["dist"], d["ins"], d["Tf"], d["Ti"], d["gagg"], d["w"], absolute=True)
    certify("g_dist", [w2, one(d["gagg"]), one(d["ins"]), one(d["Tf"])], a[0], r[0])
    certify("g_ins", [w2, p, one(d["gagg"]), one(d["Tf"])], a[1], r[1])
    certify("g_T_fwd", [w2, p, one(d["gagg"]), one(d["ins"])], a[2], r[2])
    certify("g_T_inv", [w2, p, one(d["gagg"]), one(d["ins"])], a[3], r[3])
    tl = {}
    for wrel in (None, d["wrel"]):
        tl[wrel is not None] = ref_typelayer_backward(g, d["gn"], wrel)
        certify("typelayer g_T", [one(d["gn"])] + ([(wrel, 0.5)] if wrel is not None else []),
                ref_typelayer_backward(g, d["gn"], wrel, absolute=True), tl[wrel is not None])
    return fused, r, tl


def unfused_data(I, D, weights, exact=True):
    g = graph("ladder32")
    rng = np.random.default_rng(1000 + 10 * I + D + (500 if weights else 0) + (7 if exact else 0))
    if exact:
        dist, w = exact_priors(g, rng), (exact_weights(g, rng) if weights else None)
        Tf, Ti, ins = exact_ints(rng, (g.R, D), 3), exact_ints(rng, (g.R, D), 3), exact_ints(rng, (g.B, I, D), 3)
    else:
        dist, w = random_priors(g, rng), ((0.5 + rng.random(g.F)).astype(np.float32) if weights else None)
        Tf, Ti, ins = (rng.standard_normal(s).astype(np.float32) for s in ((g.R, D), (g.R, D), (g.B, I, D)))
    return g, dist, ins, Tf, Ti, w


def typelayer_data(D, weights, exact=True, gname="ladder32"):
    g = graph(gname)
    rng = np.random.default_rng(2000 + D + (500 if weights else 0) + (7 if exact else 0))
    if exact:
        return g, exact_ints(rng, (g.R, D), 3), (exact_weights(g, rng) if weights else None)
    return g, rng.standard_normal((g.R, D)).astype(np.float32), ((0.5 + rng.random(g.F)).astype(np.float32) if weights else None)


def frontier_data(case, exact=True):
    """(graph, dist, P, w, D).  Seeds are few nodes with a non-zero prior."""
    gname = {"one_seed": "ladder32", "reaches_4097_row": "frontier_hub", "more_seeds_than_the_list": "frontier_wide",
             "sentinel": "relcounts"}[case]
    g = graph(gname)
    D = 200
    rng = np.random.default_rng(3000 + len(case) + (7 if exact else 0))
    dense = exact_priors(g, rng) if exact else random_priors(g, rng)
    dense[dense == 0] = 2.0 ** -10 if exact else 1e-6
    dist = np.zeros_like(dense)
    if case == "more_seeds_than_the_list":
        dist[0, :2060] = dense[0, :2060]                       # 2060 > 2048 seeds in question 0, three in question 1
        dist[1, [0, 17, 2099]] = dense[1, [0, 17, 2099]]
    elif case == "reaches_4097_row":
        for q in range(g.B):                                   # two light sources of the 4097-fact row
            hub = q * g.N + int(np.argmax((g.len0 + g.len1)[q * g.N:(q + 1) * g.N]))
            nb = np.unique(np.r_[g.h[g.t == hub], g.t[g.h == hub]])
            nb = nb[nb != hub][:2]
            dist.reshape(-1)[nb] = dense.reshape(-1)[nb]
    else:
        for q in range(g.B):
            deg = (g.len0 + g.len1)[q * g.N:(q + 1) * g.N]
            cand = np.flatnonzero((deg > 0) & (deg <= 64))
            pick = cand[:: max(1, len(cand) // 3)][:3] if case == "sentinel" else cand[:1]
            dist[q, pick] = dense[q, pick]
    P = exact_ints(rng, (2, g.rel_total, D), 4) if exact else rng.standard_normal((2, g.rel_total, D)).astype(np.float32)
    w = None
    if case == "reaches_4097_row":
        w = exact_weights(g, rng) if exact else (0.5 + rng.random(g.F)).astype(np.float32)
    return g, dist, P, w, D


def backward_data(gname, D, exact=True, I=2):
    """Inputs of the three backward entry points on one graph.  Exact family: the ranges of the tables and of the
    instructions are cut to [-1, 1] and [-2, 2] (the certificate at the 10 244-fact row decides, not the row)."""
    g = graph(gname)
    rng = np.random.default_rng(4000 + D + len(gname) + (7 if exact else 0))
    if exact:
        d = dict(dist=exact_priors(g, rng), w=exact_weights(g, rng), P=exact_ints(rng, (2, g.rel_total, D), 2),
                 gn=exact_ints(rng, (g.B * g.N, D), 3), Tf=exact_ints(rng, (g.R, D), 1), Ti=exact_ints(rng, (g.R, D), 1),
                 ins=exact_ints(rng, (g.B, I, D), 2), gagg=exact_ints(rng, (g.B * g.N, 2 * I * D), 3),
                 wrel=exact_weights(g, rng))
    else:
        n = lambda *s: rng.standard_normal(s).astype(np.float32)
        d = dict(dist=random_priors(g, rng), w=(0.5 + rng.random(g.F)).astype(np.float32), P=n(2, g.rel_total, D),
                 gn=n(g.B * g.N, D), Tf=n(g.R, D), Ti=n(g.R, D), ins=n(g.B, I, D), gagg=n(g.B * g.N, 2 * I * D),
                 wrel=(0.5 + rng.random(g.F)).astype(np.float32))
    return g, d
