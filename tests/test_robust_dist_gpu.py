"""Multi-Krum and the geometric median on the GPU (csrc/kernels/robust_dist.hip through ``ops.kernels`` and
``parallel.robust_dist.robust_dist_aggregate_``): the pair sums against the float64 oracle within a derived
bound, each finalizer against its host mirror fed the device's own sums, the weighted mean bitwise against
the torch specification with the device's weights, canaries around every buffer a kernel writes (``_buf``),
determinism, launch-geometry independence, a real model arena (with and without a server optimizer), and the
binding's refusals.

Every stage takes its input from the device's previous stage: the lanes add fp32 squares, the oracle adds
in fp64, so a discrete decision (which clients multi-Krum selects) is never compared across the two
summation orders -- only given the same distances."""
import math
import types

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, GraphedTrainStep, make_step_fn)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier, DistilBertConfig)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as K
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.parallel import (
    robust as rb, robust_dist as rd, server_opt as so)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N1 = 1024                                # 256 float4: one block
N2 = 1028                                # 257 float4: a second block with one live lane
N_WRAP = 4 * (4096 * 256 + 256)          # one block above a full sweep of the 4 096-block grid
MAX_M = 16
PADS = (0, 512, N1 - 64)                 # 64-float alignment pads: +0 in every client
CTL, KS, ROW = 20, 288, 34
U = 2.0 ** -24
NAN = float("nan")


def _make(n, M, pads, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = 0.05 * torch.randn(n, device=DEV, generator=g)
    states = [base + 1e-3 * torch.randn(n, device=DEV, generator=g) for _ in range(M)]
    for s in states:
        for p in pads:
            s[p:p + 64] = 0.0
    return states


@pytest.fixture(scope="module")
def clients():
    """16 clients' vectors of N2 floats, 0.05 N(0, 1) + 1e-3 N(0, 1) per client; computed once, never
    written (a test that changes a client clones it)."""
    return _make(N2, MAX_M, PADS, 23)


def _terms(n):
    """T: the most squares one lane adds over n floats (4 per float4, one float4 per sweep of the grid)."""
    n4 = n // 4
    return 4 * -(-n4 // (256 * K.robust_dist_grid(n)))


def _bound(n):
    return (_terms(n) + 4) * U


GUARD = 64                               # canary elements on either side of every buffer a kernel writes
_CANARY = {torch.float64: -77.0, torch.float32: 1234.5, torch.bfloat16: 7.0}
_guarded = []                            # (whole allocation, numel of the window) since the last _check_guards


def _buf(numel, dtype, fill):
    """A window of ``numel`` elements filled with ``fill`` between two GUARD-element canaries."""
    big = torch.full((numel + 2 * GUARD,), _CANARY[dtype], dtype=dtype, device=DEV)
    win = big[GUARD:GUARD + numel]
    win.fill_(fill)
    _guarded.append((big, numel))
    return win


def _check_guards():
    """Every canary of every window handed out since the last call is intact (stream-ordered after the
    launches that wrote the windows)."""
    assert _guarded
    for big, numel in _guarded:
        c = _CANARY[big.dtype]
        assert bool((big[:GUARD] == c).all()) and bool((big[GUARD + numel:] == c).all()), (big.dtype, numel)
    _guarded.clear()


def _intact(*windows):
    """The canaries of these ``_buf`` windows are intact (for buffers that outlive one launch)."""
    for w in windows:
        big, c = w._base, _CANARY[w.dtype]
        assert bool((big[:GUARD] == c).all()) and bool((big[GUARD + w.numel():] == c).all()), (w.dtype, w.numel())


def _geomed_finalize(pt, grid, M, nu, it, ctl, stats):
    """The Weiszfeld finalizer into ``_buf`` windows: canaries intact, and the stats rows other than ``it``
    exactly as they were."""
    before = stats.clone()
    K.robust_geomed_finalize(pt, grid, M, nu, it, ctl, stats)
    _intact(ctl, stats)
    keep = torch.ones(stats.numel(), dtype=torch.bool, device=DEV)
    keep[it * ROW:(it + 1) * ROW] = False
    assert torch.equal(stats.view(torch.int64)[keep], before.view(torch.int64)[keep]), (M, it)


def _pairdist(states):
    M, n = len(states), states[0].numel()
    grid, P = K.robust_dist_grid(n), M * (M - 1) // 2
    part = _buf(grid * P, torch.float64, NAN)
    K.robust_pairdist(states, part)
    _check_guards()
    return part, grid


def _block_order_sum(part, grid, ncols):
    """The block partials of every column added in the finalizers' fixed order (robust_dist.hip
    reduce_columns): R = min(16, 256 // ncols) ranks, rank r adds the blocks r, r + R, ... in that order
    from 0.0, then the rank sums are added in rank order from 0.0."""
    rows = part.view(grid, ncols).cpu()
    R = min(16, 256 // ncols)
    total = torch.zeros(ncols, dtype=torch.float64)
    for r in range(R):
        acc = torch.zeros(ncols, dtype=torch.float64)
        for b in range(r, grid, R):
            acc = acc + rows[b]
        total = total + acc
    return total.tolist()


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _matrix(part, grid, M):
    cols = part.view(grid, M * (M - 1) // 2).sum(dim=0).tolist()
    D = [[0.0] * M for _ in range(M)]
    for i in range(M):
        for j in range(i + 1, M):
            D[i][j] = D[j][i] = cols[i * (2 * M - i - 1) // 2 + (j - i - 1)]
    return D


def _krum(states, f, m):
    """pairdist -> krum_finalize on the device: (ctl, stats) as tensors."""
    return _krum_from(states, f, m)[:2]


def _krum_from(states, f, m):
    """As ``_krum``, with the partials the finalizer read: (ctl, stats, part, grid)."""
    part, grid = _pairdist(states)
    ctl = _buf(CTL, torch.float32, NAN)
    stats = _buf(KS, torch.float64, NAN)
    K.robust_krum_finalize(part, grid, len(states), f, m, ctl, stats)
    _check_guards()
    return ctl, stats, part, grid


def _bits32(values):
    return torch.tensor(values, dtype=torch.float32).view(torch.int32).tolist()


def _check_krum(states, f, m):
    """The finalizer against ``krum_select`` fed the device's own D, bit for bit: scores, mask, weights, flag."""
    M = len(states)
    ctl, stats, part, grid = _krum_from(states, f, m)
    st, c = stats.tolist(), ctl.tolist()
    D = [st[16 * i:16 * i + M] for i in range(M)]
    # D is the fixed-order sum of the partials it was reduced from, pair (i < j) at its index: both sides
    # add the same doubles in the same order, so the comparison is exact at any grid
    cols = _block_order_sum(part, grid, M * (M - 1) // 2)
    for i in range(M):
        for j in range(i + 1, M):
            want = cols[i * (2 * M - i - 1) // 2 + (j - i - 1)]
            assert _same(D[i][j], want) and _same(D[j][i], want), (M, i, j)
    scores, selected, weights, flag = rd.krum_select(D, f, m)
    assert torch.tensor(st[256:256 + M], dtype=torch.float64).view(torch.int64).tolist() == \
        torch.tensor(scores, dtype=torch.float64).view(torch.int64).tolist(), (M, f, m)
    assert [i for i in range(M) if st[272 + i] == 1.0] == selected and set(st[272:288]) <= {0.0, 1.0}
    assert _bits32(c[:M]) == _bits32(weights) and not any(_bits32(c[M:16])) and c[17:] == [0.0] * 3
    assert c[16] == float(flag)
    for i in range(16):                  # D: symmetric, diagonal and unused rows / columns 0
        for j in range(16):
            d = st[16 * i + j]
            if i >= M or j >= M or i == j:
                assert d == 0.0
            else:
                e = st[16 * j + i]
                assert d == e or (math.isnan(d) and math.isnan(e))
    return scores, selected, weights, flag, D


def _wmean(states, ctl, out=True, shadow=True, partial=True):
    M, n = len(states), states[0].numel()
    o = _buf(n, torch.float32, NAN) if out else None
    sh = _buf(n, torch.bfloat16, 3.0) if shadow else None
    pt = _buf((M + 1) * K.robust_dist_grid(n), torch.float64, NAN) if partial else None
    K.robust_wmean(states, ctl, o, sh, pt)
    _check_guards()
    return o, sh, pt


def _check_wmean(states, ctl, o, sh, pt):
    """out / shadow bitwise against the specification with the device's weights; the distances against
    fp64 from the device's own out within the pair-sum bound; the non-finite count exact."""
    M, n = len(states), states[0].numel()
    want, _, nonfinite = rd.torch_weighted_mean_(states, ctl[:M])
    assert torch.equal(o.view(torch.int32), want.view(torch.int32)), M
    if sh is not None:
        assert torch.equal(sh.view(torch.int16), o.to(torch.bfloat16).view(torch.int16)), M
    sums = pt.view(-1, M + 1).sum(dim=0).tolist()
    assert sums[M] == float(nonfinite), M
    worst = 0.0
    for i, x in enumerate(states):
        ref = float(((x.double() - o.double()) ** 2).sum())
        if math.isfinite(ref) and ref < 1e38:
            dev = abs(sums[i] - ref) / ref if ref > 0.0 else abs(sums[i])
            worst = max(worst, dev)
            assert dev <= _bound(n), (M, i, dev, _bound(n))
        else:
            assert not math.isfinite(sums[i]), (M, i)
    return want, worst


# ------------------------------------------------------------------ pair sums
@pytest.mark.parametrize("M", list(range(2, MAX_M + 1)))
def test_pairdist_against_the_float64_oracle(M, clients):
    """Relative bound (T + 4) 2^-24, T the most terms one lane adds.  Derivation, u = 2^-24: a term is
    fl(fl(x_i - x_j)^2) -- one rounding for the difference (relative u on d, 2u on d^2) and one for the
    square: at most 3u + O(u^2) off (x_i - x_j)^2.  A lane adds its T non-negative terms one by one:
    T - 1 roundings, each at most u relative to a partial sum that never exceeds the final one, so
    (T - 1) u.  All terms are >= 0, so the relative error of the whole sum is at most that of its worst
    lane: (T + 2) u + O(T u^2); the fp64 steps (conversion is exact; 6 shuffle adds, 3 LDS adds, <= 4 096
    block adds at 2^-53 each) stay below 2^-40.  (T + 4) u covers both remainders; here T = 4 (one float4
    per lane), so the bound is 8 u = 4.8e-7.
    Measured worst deviation over M = 2 .. 16 and both lengths: 1.2e-8 (40 times inside the bound: the
    clients differ by 1e-3 of their values, so most differences are exact and the roundings do not line up);
    at the wrapped length (T = 8, bound 7.2e-7) 2.7e-10, and 1.2e-8 for the distances of ``robust_wmean``
    (M = 2 .. 16)."""
    assert K.robust_dist_grid(N1) == 1 and K.robust_dist_grid(N2) == 2 == K.server_opt_grid(N2)
    assert _terms(N1) == _terms(N2) == 4
    worst = 0.0
    for n in (N1, N2):
        states = [s[:n] for s in clients[:M]]
        part, grid = _pairdist(states)
        assert bool(torch.isfinite(part).all())          # (every entry of every block row was written)
        D = _matrix(part, grid, M)
        want = rd.torch_pair_sqdist(states).tolist()
        for i in range(M):
            for j in range(M):
                if i != j:
                    dev = abs(D[i][j] - want[i][j]) / want[i][j]
                    worst = max(worst, dev)
                    assert dev <= _bound(n), (M, n, i, j, dev)
    print(f"pairdist M={M}: worst relative deviation {worst:.3e} of bound {_bound(N2):.3e}")


@pytest.mark.parametrize("M", [3, MAX_M])
def test_grid_wrap(M):
    """One block above a full sweep of the capped grid: the lanes of block 0 make two iterations (T = 8)."""
    states = _make(N_WRAP, M, (0, 64 * 40001, N_WRAP - 64), 200 + M)
    assert K.robust_dist_grid(N_WRAP) == 4096 and _terms(N_WRAP) == 8
    part, grid = _pairdist(states)
    D = _matrix(part, grid, M)
    want = rd.torch_pair_sqdist(states).tolist()
    worst = max(abs(D[i][j] - want[i][j]) / want[i][j] for i in range(M) for j in range(M) if i != j)
    print(f"pairdist wrap M={M}: worst relative deviation {worst:.3e} of bound {_bound(N_WRAP):.3e}")
    assert worst <= _bound(N_WRAP)
    f = rd.default_byzantine(M)
    scores, selected, weights, flag, _ = _check_krum(states, f, M - f)
    assert flag == 0 and len(selected) == M - f
    ctl, _ = _krum(states, f, M - f)
    o, sh, pt = _wmean(states, ctl)
    _, w = _check_wmean(states, ctl, o, sh, pt)
    print(f"wmean wrap M={M}: worst relative distance deviation {w:.3e}")
    for p in (0, 64 * 40001, N_WRAP - 64):
        assert not o[p:p + 64].view(torch.int32).any()


# ------------------------------------------------------------------ the Krum finalizer
def test_krum_finalize_equals_its_host_mirror(clients):
    for M in range(2, MAX_M + 1):
        f = rd.default_byzantine(M)
        for m in sorted({1, M - f}):
            scores, selected, weights, flag, _ = _check_krum(clients[:M], f, m)
            assert flag == 0 and len(selected) == m and all(math.isfinite(s) for s in scores)
    _check_krum(clients[:8], 0, 8)       # c = 6
    _check_krum(clients[:8], 5, 3)       # c = 1
    _check_krum(clients[:3], 7, 1)       # c = max(1, .)


def test_krum_finalize_tie_goes_to_the_lower_slot(clients):
    """Slots 1 and 4 hold the same vector: their rows of D, hence their scores, are equal bit for bit, and
    with the cut between them the lower slot is taken."""
    states = [s.clone() for s in clients[:6]]
    states[4] = states[1].clone()
    scores, _, _, _, _ = _check_krum(states, 1, 6)
    assert scores[1] == scores[4]
    order = sorted(range(6), key=lambda i: (scores[i], i))
    m = order.index(1) + 1
    assert order[m] == 4
    _, selected, weights, flag, _ = _check_krum(states, 1, m)
    assert 1 in selected and 4 not in selected and weights[4] == 0.0 and flag == 0


def test_krum_finalize_nan_overflow_and_too_few(clients):
    states = [s.clone() for s in clients[:8]]
    states[2].fill_(NAN)
    states[5].fill_(3e30)                # (3e30 - x)^2 overflows fp32: the pair sums are inf
    scores, selected, weights, flag, D = _check_krum(states, 2, 6)
    assert flag == 0 and selected == [0, 1, 3, 4, 6, 7]
    assert scores[2] == math.inf and scores[5] == math.inf and all(math.isfinite(scores[i]) for i in selected)
    assert math.isnan(D[2][0]) and D[5][0] == math.inf
    # one more client asked for than has a finite score
    scores, selected, weights, flag, _ = _check_krum(states, 2, 7)
    assert flag == 1 and selected == [] and weights == [0.0] * 8
    # two NaN clients of four, f = 0: every client's two nearest include a NaN client
    four = [s.clone() for s in clients[:4]]
    four[0].fill_(NAN)
    four[3].fill_(NAN)
    scores, selected, weights, flag, _ = _check_krum(four, 0, 2)
    assert flag == 1 and scores == [math.inf] * 4


# ------------------------------------------------------------------ the weighted mean
@pytest.mark.parametrize("M", list(range(2, MAX_M + 1)))
def test_wmean_equals_the_specification(M, clients):
    worst = 0.0
    for n in (N1, N2):
        states = [s[:n] for s in clients[:M]]
        f = rd.default_byzantine(M)
        ctl, stats = _krum(states, f, M - f)
        assert float(ctl[16]) == 0.0 and int((ctl[:M] != 0).sum()) == M - f
        o, sh, pt = _wmean(states, ctl)
        _, w = _check_wmean(states, ctl, o, sh, pt)
        worst = max(worst, w)
        for p in PADS:
            assert not o[p:p + 64].view(torch.int32).any(), (M, p)
        # out omitted: the distances and the count alone, equal to those of the full launch
        _, _, pt2 = _wmean(states, ctl, out=False, shadow=False)
        assert torch.equal(pt2.view(torch.int64), pt.view(torch.int64))
        # no partial: the same out
        o3, sh3, _ = _wmean(states, ctl, partial=False)
        assert torch.equal(o3.view(torch.int32), o.view(torch.int32)) and torch.equal(sh3.view(torch.int16), sh.view(torch.int16))
    print(f"wmean M={M}: worst relative distance deviation {worst:.3e} of bound {_bound(N2):.3e}")


def test_wmean_skips_a_zero_weight_nan_slot(clients):
    states = [s.clone() for s in clients[:5]]
    states[0].fill_(NAN)                 # (slot 0: the first non-zero weight is not the first slot)
    states[3].fill_(NAN)
    ctl, _ = _krum(states, 1, 3)
    assert ctl[:5].tolist() == [0.0, rb.f32(1 / 3), rb.f32(1 / 3), 0.0, rb.f32(1 / 3)]
    o, sh, pt = _wmean(states, ctl)
    want, _ = _check_wmean(states, ctl, o, sh, pt)
    assert bool(torch.isfinite(o).all())
    sums = pt.view(-1, 6).sum(dim=0).tolist()
    assert math.isnan(sums[0]) and math.isnan(sums[3]) and sums[5] == 0.0
    # a NaN weight-bearing slot is counted: every output is NaN
    ctl2 = ctl.clone()
    ctl2[3] = 0.25
    o, sh, pt = _wmean(states, ctl2)
    assert pt.view(-1, 6).sum(dim=0).tolist()[5] == float(N2) and bool(torch.isnan(o).all())
    # all weights zero: +0, and the distances are the squared norms
    o, sh, pt = _wmean(states, torch.zeros(CTL, device=DEV))
    assert not o.view(torch.int32).any() and not sh.view(torch.int16).any()
    _check_wmean(states, torch.zeros(CTL, device=DEV), o, sh, pt)


def test_wmean_sum_order_is_the_slot_order(clients):
    """Geometric-median weights (all different): the fp32 sum in slot order is not the sum in reverse order,
    and the kernel equals the former bit for bit."""
    M = 8
    states = [s.clone() for s in clients[:M]]
    states[6] = states[6] * -4.0
    ctl = _buf(CTL, torch.float32, 0.0)
    _, _, pt = _wmean(states, ctl, out=False, shadow=False)
    stats = _buf(ROW, torch.float64, 0.0)
    _geomed_finalize(pt, K.robust_dist_grid(N2), M, 1e-6, 0, ctl, stats)
    assert len(set(ctl[:M].tolist())) == M
    o, sh, pt = _wmean(states, ctl)
    want, _ = _check_wmean(states, ctl, o, sh, pt)
    rev, _, _ = rd.torch_weighted_mean_(states[::-1], ctl[:M].flip(0))
    assert not torch.equal(rev.view(torch.int32), want.view(torch.int32))


def test_wmean_writes_nothing_when_refused(clients):
    """flag = 1 in ctl (too few finite scores): out, shadow and partial keep their contents, canaries too."""
    four = [s.clone() for s in clients[:4]]
    four[0].fill_(NAN)
    four[3].fill_(NAN)
    ctl, _ = _krum(four, 0, 2)
    assert float(ctl[16]) == 1.0
    C, grid = 64, K.robust_dist_grid(N2)
    obig = torch.full((N2 + 2 * C,), 1234.5, device=DEV)
    sbig = torch.full((N2 + 2 * C,), 7.0, dtype=torch.bfloat16, device=DEV)
    pbig = torch.full((5 * grid + 2 * C,), -77.0, dtype=torch.float64, device=DEV)
    K.robust_wmean(four, ctl, obig[C:C + N2], sbig[C:C + N2], pbig[C:C + 5 * grid])
    torch.cuda.synchronize()
    assert torch.equal(obig, torch.full_like(obig, 1234.5)) and torch.equal(sbig, torch.full_like(sbig, 7.0))
    assert torch.equal(pbig, torch.full_like(pbig, -77.0))


# ------------------------------------------------------------------ the Weiszfeld finalizer
def _ulps(a, b):
    ia = torch.tensor(a, dtype=torch.float64).view(torch.int64)
    ib = torch.tensor(b, dtype=torch.float64).view(torch.int64)
    return int((ia - ib).abs().max())


def test_geomed_finalize_equals_its_host_mirror(clients):
    """Weights and objective against ``geomed_weights`` fed the device's Dz, over four passes, each pass's
    weights taken from the device's previous stage.  fp64 sqrt and division are correctly rounded on this
    target and the sums run in slot order on both sides, so the comparison is bitwise: the fp64 quotients
    in the stats row, the objective, and the fp32 weights in ctl."""
    worst = 0
    for M in range(2, MAX_M + 1):
        states = _make(N2, M, PADS, 300 + M)
        if M >= 5:
            states[1] = states[1] * -4.0
            states[2].fill_(NAN)
            states[4].fill_(3e30)
        grid = K.robust_dist_grid(N2)
        ctl = _buf(CTL, torch.float32, 0.0)
        stats = _buf(4 * ROW, torch.float64, NAN)
        for it in range(4):
            _, _, pt = _wmean(states, ctl, out=False, shadow=False)
            _geomed_finalize(pt, grid, M, 1e-6, it, ctl, stats)
            assert bool(torch.isnan(stats[(it + 1) * ROW:]).all())   # (the rows not yet written)
            row, c = stats[it * ROW:(it + 1) * ROW].tolist(), ctl.tolist()
            Dz = row[2:2 + M]
            cols = _block_order_sum(pt, grid, M + 1)
            assert all(_same(a, b) for a, b in zip(Dz, cols[:M])) and row[1] == cols[M], (M, it)
            beta, objective, flag, beta64 = rd.geomed_weights(Dz, 1e-6)
            worst = max(worst, _ulps(row[18:18 + M], beta64), _ulps([row[0]], [objective]))
            assert row[18:18 + M] == beta64 and row[0] == objective, (M, it)
            assert _bits32(c[:M]) == _bits32(beta) and not any(_bits32(c[M:16])), (M, it)
            assert c[16] == float(flag) == 0.0 and c[17:] == [0.0] * 3 and row[1] == 0.0
            assert row[2 + M:18] == [0.0] * (16 - M) and row[18 + M:] == [0.0] * (16 - M)
            if M >= 5:
                assert c[2] == 0.0 and c[4] == 0.0 and 0.0 < c[1] < 1.0 / M
    print(f"geomed_finalize: worst distance to the host mirror {worst} ulp of fp64")
    # nobody usable: flag = 1 and every weight 0
    bad = [torch.full((N1,), NAN, device=DEV), torch.full((N1,), 3e30, device=DEV)]
    ctl = _buf(CTL, torch.float32, 0.0)
    _, _, pt = _wmean(bad, ctl, out=False, shadow=False)
    stats = _buf(ROW, torch.float64, 0.0)
    _geomed_finalize(pt, 1, 2, 1e-6, 0, ctl, stats)
    assert ctl.tolist() == [0.0] * 16 + [1.0, 0.0, 0.0, 0.0] and rd.geomed_weights(stats[2:4], 1e-6)[2] == 1
    # nu is the floor of a distance: two equal clients sit on the centre after one pass
    same = [clients[0][:N1].clone(), clients[0][:N1].clone()]
    ctl = _buf(CTL, torch.float32, 0.0)
    ctl[0] = 1.0
    _, _, pt = _wmean(same, ctl, out=False, shadow=False)
    _geomed_finalize(pt, 1, 2, 1e-6, 0, ctl, stats)
    assert ctl[:2].tolist() == [0.5, 0.5] and float(stats[0]) == 0.0


# ------------------------------------------------------------------ the whole aggregate
class FlatModel:
    """What ``robust_dist_aggregate_`` needs of a model: a flat fp32 master and a bf16 shadow."""

    def __init__(self, master, pad=64):
        self.mbig = torch.full((master.numel() + 2 * pad,), 1234.5, device=DEV)
        self.sbig = torch.full((master.numel() + 2 * pad,), 7.0, dtype=torch.bfloat16, device=DEV)
        m, s = self.mbig[pad:-pad], self.sbig[pad:-pad]
        m.copy_(master)
        s.copy_(master.to(torch.bfloat16))
        self.arena = types.SimpleNamespace(master=m, shadow=s)
        self.pad, self.synced = pad, 0

    def mark_shadow_synced(self):
        self.synced += 1

    def canaries_intact(self):
        p = self.pad
        return (bool((self.mbig[:p] == 1234.5).all()) and bool((self.mbig[-p:] == 1234.5).all())
                and bool((self.sbig[:p] == 7.0).all()) and bool((self.sbig[-p:] == 7.0).all()))


@pytest.mark.parametrize("kind", rd.DIST_AGGREGATORS)
def test_whole_aggregate_canaries_and_determinism(kind, clients):
    states = [s.clone() for s in clients[:8]]
    states[3] = states[3] * -4.0
    states[6].fill_(NAN)
    runs = []
    for _ in range(2):
        model = FlatModel(torch.zeros(N2, device=DEV))
        rep = rd.robust_dist_aggregate_(model, states, kind, byzantine=2)
        torch.cuda.synchronize()
        assert model.canaries_intact() and model.synced == 1
        runs.append((model.arena.master.clone(), model.arena.shadow.clone(), rep))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16))
    assert repr(runs[0][2]) == repr(runs[1][2])
    out, sh, rep = runs[0]
    assert bool(torch.isfinite(out).all()) and torch.equal(sh.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))
    for i in (0, 1, 2, 4, 5, 7):
        assert torch.equal(states[i], clients[i])        # (the sources are not written)
    if kind == "multi_krum":
        assert rep["rejected"] == [3, 6] and rep["selected"] == [0, 1, 2, 4, 5, 7] and (rep["f"], rep["m"]) == (2, 6)
        assert rep["scores"][6] == math.inf and rep["scores"][3] > 100 * max(rep["scores"][i] for i in rep["selected"])
        weights = [rb.f32(1 / 6) if i in rep["selected"] else 0.0 for i in range(8)]
    else:
        weights = rep["weights"]
        assert weights[6] == 0.0 and 0.0 < weights[3] < 0.1 / 8 and len(rep["objective"]) == 7
        obj = rep["objective"]
        assert all(obj[i + 1] <= obj[i] * (1 + 1e-6) for i in range(1, 6))
    want, _, _ = rd.torch_weighted_mean_(states, weights)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    # out is independent of the launch geometry: the same weights on windows of the vectors
    ctl = torch.zeros(CTL, device=DEV)
    ctl[:8] = torch.tensor(weights, device=DEV)
    for a, b in ((0, 1024), (4, 8), (512, N2), (1024, N2)):
        o, s2, _ = _wmean([s[a:b] for s in states], ctl, partial=False)
        assert torch.equal(o.view(torch.int32), out[a:b].view(torch.int32)), (a, b)
        assert torch.equal(s2.view(torch.int16), sh[a:b].view(torch.int16)), (a, b)


@pytest.mark.parametrize("kind", rd.DIST_AGGREGATORS)
def test_too_many_liars_leave_the_master_as_it_was(kind, clients):
    states = [torch.full((N2,), NAN, device=DEV) for _ in range(4)]
    if kind == "multi_krum":
        states[1] = clients[1].clone()                   # one honest client among NaNs: every score is inf
    start = clients[0].clone()
    model = FlatModel(start)
    srv = so.ServerOptimizer(model, "adam", lr=0.01)
    with pytest.raises(RuntimeError, match="left the model as it was.*slot 0"):
        rd.robust_dist_aggregate_(model, states, kind, srv)
    torch.cuda.synchronize()
    assert torch.equal(model.arena.master.view(torch.int32), start.view(torch.int32)) and model.canaries_intact()
    assert torch.equal(model.arena.shadow.view(torch.int16), start.to(torch.bfloat16).view(torch.int16))
    assert srv.rounds == 0 and model.synced == 0
    with pytest.raises(ValueError, match="at most 16"):
        rd.robust_dist_aggregate_(model, [clients[0]] * 17, kind)
    with pytest.raises(ValueError, match="byzantine"):
        rd.robust_dist_aggregate_(model, list(clients[:6]), "multi_krum", byzantine=2)
    one = FlatModel(start)
    rep = rd.robust_dist_aggregate_(one, [clients[5]], kind)
    assert torch.equal(one.arena.master, clients[5]) and rep["clients"] == 1 and rep["kind"] == kind
    assert torch.equal(one.arena.shadow.view(torch.int16), clients[5].to(torch.bfloat16).view(torch.int16))


def _batch(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(S // 3, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids = ids * mask
    ids[:, 0] = 101
    labels = torch.randint(0, 2, (B,), generator=g)
    return ids.cuda(), mask.cuda(), labels.cuda(), int(lens.sum())


@pytest.mark.parametrize("with_server", [False, True])
@pytest.mark.parametrize("kind", rd.DIST_AGGREGATORS)
def test_aggregate_on_a_model_arena(kind, with_server):
    """``RobustAggregator.aggregate_`` of 5 perturbed copies of a one-layer DistilBERT arena, client 1 sending
    ``-4 w`` and client 3 NaN: the master is the specification's weighted mean with the reported weights (or,
    with a server optimizer, the fp32 chain's step on it), the shadow is the master's, the pads stay +0, the
    liars are named, and a graphed training step runs on the result."""
    model = DDoSClassifier(config=DistilBertConfig(n_layers=1), device=DEV, impl="hip", seed=3)
    A = model.arena
    x0 = A.master.clone()
    live = torch.zeros(A.numel, dtype=torch.bool, device=DEV)
    for name in A.names():
        off, shape = A.offsets[name]
        live[off:off + math.prod(shape)] = True
    assert int((~live).sum()) > 0
    g = torch.Generator(device=DEV).manual_seed(5)
    states = [x0 + 1e-3 * torch.randn(A.numel, device=DEV, generator=g) * live for _ in range(5)]
    states[1] = states[1] * -4.0
    states[3] = torch.full_like(states[3], NAN)
    server = so.ServerOptimizer(model, "adam", lr=0.01) if with_server else None
    robust = rb.RobustAggregator(kind, krum_select=3)    # (two liars of five: Krum's f = 1 needs the cut at 3)
    rep = robust.aggregate_(model, states, server)
    torch.cuda.synchronize()
    assert rep["kind"] == kind and rep["clients"] == 5
    if kind == "multi_krum":
        assert (rep["f"], rep["m"]) == (1, 3) and rep["selected"] == [0, 2, 4] and rep["rejected"] == [1, 3]
        assert rep["scores"][3] == math.inf and len(rep["distances"]) == 5 and rep["distances"][0][0] == 0.0
        weights = [rb.f32(1 / 3), 0.0, rb.f32(1 / 3), 0.0, rb.f32(1 / 3)]
    else:
        weights = rep["weights"]
        assert weights[3] == 0.0 and 0.0 < weights[1] < 0.1 / 5 and abs(sum(weights) - 1.0) < 1e-6
        assert len(rep["objective"]) == rep["iters"] + 1 == 7 and math.isnan(rep["distances"][3])
    agg, _, nonfinite = rd.torch_weighted_mean_(states, weights)
    assert nonfinite == 0
    if with_server:
        x, m = x0.clone(), torch.zeros_like(x0)
        v = torch.full_like(x0, so.f32(server.tau * server.tau))
        so.torch_chain_("adam", agg, x, m, v, 1.0, server.lr, server.b1, server.b2, server.tau)
        # the bound of tests/test_robust_agg_gpu.py: the aggregate fed to both is the same bits; kernel and
        # chain each round x' once and their steps differ by a few roundings of sqrt / divide
        assert float((A.master.double() - x.double()).abs().max()) <= 4 * U * float(x.abs().max())
        assert torch.equal(server.x, A.master) and server.rounds == 1
    else:
        assert torch.equal(A.master.view(torch.int32), agg.view(torch.int32))
    assert torch.equal(A.shadow.view(torch.int16), A.master.to(torch.bfloat16).view(torch.int16))
    assert not A.master[~live].view(torch.int32).any()
    model.train()
    opt = ArenaAdam(model, lr=1e-3)
    opt.reset_state()
    ids, mask, labels, tokens = _batch(16, 128, seed=1)
    st = GraphedTrainStep(make_step_fn(model, opt), warmup=1, bucket=model.packed_rows)
    before = A.master.clone()
    losses = [float(st(ids, mask, labels, tokens)) for _ in range(3)]
    torch.cuda.synchronize()
    assert st.failed is None and len(st.graphs) >= 1 and all(math.isfinite(v) for v in losses)
    assert not torch.equal(A.master, before)


# ------------------------------------------------------------------ the binding
def test_refusals():
    """The binding rejects each invalid call before any launch: the buffers keep their contents."""
    n = 2048
    grid = K.robust_dist_grid(n)
    mk = lambda k=n, dt=torch.float32: torch.ones(k, dtype=dt, device=DEV)  # noqa: E731
    srcs = [mk(), mk(), mk()]
    out, sh = mk(), mk(dt=torch.bfloat16)
    pp, wp = mk(3 * grid, torch.float64), mk(4 * grid, torch.float64)
    ctl, ks, gs = torch.zeros(CTL, device=DEV), mk(KS, torch.float64), mk(2 * ROW, torch.float64)
    ext = K.ext()

    def bad(fn, ok, **kw):
        with pytest.raises(RuntimeError):
            fn(**dict(ok, **kw))

    ok = dict(srcs=srcs, partial=pp)
    bad(ext.robust_pairdist, ok, srcs=[mk()])
    bad(ext.robust_pairdist, ok, srcs=[mk() for _ in range(17)])
    bad(ext.robust_pairdist, ok, srcs=[mk(n - 2)] * 3)                 # numel % 4
    bad(ext.robust_pairdist, ok, srcs=[mk(), mk(dt=torch.float64), mk()])
    bad(ext.robust_pairdist, ok, srcs=[mk(), mk(2 * n)[::2], mk()])    # not contiguous
    bad(ext.robust_pairdist, ok, srcs=[mk(), mk(n - 4), mk()])
    bad(ext.robust_pairdist, ok, srcs=[mk(), mk().cpu(), mk()])
    bad(ext.robust_pairdist, ok, partial=pp[:-1])
    bad(ext.robust_pairdist, ok, partial=pp.float())
    ok = dict(partial=pp, grid=grid, M=3, f=0, m=3, ctl=ctl, stats=ks)
    for kw in (dict(M=1), dict(M=17), dict(M=4), dict(f=-1), dict(m=0), dict(m=4), dict(grid=0), dict(grid=grid + 1),
               dict(grid=4097), dict(ctl=ctl[:19]), dict(stats=ks[:-1]), dict(ctl=ctl.double()), dict(stats=ks.float()),
               dict(partial=pp.float()), dict(ctl=ctl.cpu())):
        bad(ext.robust_krum_finalize, ok, **kw)
    ok = dict(srcs=srcs, ctl=ctl, out=out, shadow=sh, partial=wp)
    big = mk(2 * n)
    for kw in (dict(srcs=[mk()]), dict(srcs=[mk() for _ in range(17)]), dict(out=None), dict(ctl=ctl[:16]),
               dict(ctl=ctl.double()), dict(out=mk(n + 4)), dict(out=mk(dt=torch.bfloat16)), dict(shadow=mk()),
               dict(shadow=mk(n - 4, torch.bfloat16)), dict(partial=wp[:-1]), dict(partial=wp.float()),
               dict(srcs=[mk(), mk(n - 4), mk()]), dict(srcs=[mk(), mk().cpu(), mk()]), dict(out=srcs[1]),
               dict(srcs=[mk(), big[:n], mk()], out=big[n // 2:n // 2 + n]),
               dict(srcs=[mk(), big[:n], mk()], shadow=big[n // 2:n].view(torch.bfloat16))):
        bad(ext.robust_wmean, ok, **kw)
    ok = dict(partial=wp, grid=grid, M=3, nu=1e-6, iter=0, ctl=ctl, stats=gs)
    for kw in (dict(M=1), dict(M=17), dict(M=4), dict(nu=0.0), dict(nu=-1.0), dict(nu=NAN), dict(nu=math.inf),
               dict(iter=-1), dict(iter=2), dict(grid=0), dict(grid=grid + 1), dict(ctl=ctl[:19]), dict(stats=gs.float()),
               dict(partial=wp.float())):
        bad(ext.robust_geomed_finalize, ok, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(t, torch.ones_like(t)) for t in srcs + [out, sh, pp, wp, ks, gs]) and not ctl.any()
    K.robust_wmean([mk(), big[:n], mk()], ctl, big[n:], sh, wp)       # beside a source: accepted
    torch.cuda.synchronize()
    assert not big[n:].any() and wp.view(grid, 4).sum(dim=0).tolist() == [n, n, n, 0]
