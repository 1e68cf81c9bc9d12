"""The fused robust aggregate on the GPU (csrc/kernels/robust_agg.hip through ``ops.kernels.robust_agg``
and ``parallel.robust.robust_aggregate_``): bitwise against the torch specification on the device for
every client count 2 .. 16, the grid-stride wrap, launch-geometry independence, canaries and the
counts rows, determinism, NaN / inf / signed-zero inputs, a real model arena (with and without a
server optimizer), and the binding's refusals.

Every kernel result is compared bit for bit: the kernel and ``torch_robust_`` make the same fp32
additions in the same order and one multiplication, so no tolerance applies."""
import math

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, GraphedTrainStep, make_step_fn)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as K
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.parallel import (
    robust as rb, server_opt as so)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 4000                                 # 1 000 float4: three full blocks and a partial one
N_WRAP = 4096 * 1024 + 4 * 257           # the 4 096-block grid-stride loop wraps; ragged tail
MAX_M = 16
PADS = (0, 1984, N - 64)                 # 64-float alignment pads: +0 in every client
COLS = 17


def _ks(M):
    return sorted({0, 1 if 2 * 1 < M else 0, (M - 1) // 2})


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
    """16 clients' vectors, 0.05 N(0, 1) + 1e-3 N(0, 1) per client; computed once, never written."""
    return _make(N, MAX_M, PADS, 17)


def _launch(states, k, shadow=True, counts=True):
    n = states[0].numel()
    out = torch.full((n,), float("nan"), device=DEV)
    sh = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV) if shadow else None
    ct = torch.full((COLS * K.robust_agg_grid(n),), -12345, dtype=torch.int32, device=DEV) if counts else None
    K.robust_agg(states, k, out, sh, ct)
    return out, sh, ct


def _sums(ct):
    return ct.view(-1, COLS).sum(dim=0, dtype=torch.int64)


def _check(states, k, out, sh, ct):
    M = len(states)
    want, trimmed, nonfinite = rb.torch_robust_(states, k)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (M, k)
    assert torch.equal(sh.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)), (M, k)
    sums = _sums(ct)
    assert sums[:M].tolist() == trimmed.tolist(), (M, k)
    assert not ct.view(-1, COLS)[:, M:MAX_M].any(), (M, k)
    assert int(sums[MAX_M]) == nonfinite, (M, k)
    return want, trimmed, nonfinite


@pytest.mark.parametrize("M", list(range(2, MAX_M + 1)))
def test_kernel_equals_the_specification(M, clients):
    assert K.robust_agg_grid(N) == 4 == K.server_opt_grid(N)
    states = clients[:M]
    for k in _ks(M):
        out, sh, ct = _launch(states, k)
        want, trimmed, nonfinite = _check(states, k, out, sh, ct)
        assert nonfinite == 0 and int(trimmed.sum()) == 2 * k * N
        for p in PADS:
            assert not out[p:p + 64].view(torch.int32).any(), (M, k, p)
        assert bool((ct.view(-1, COLS) >= 0).all())


@pytest.mark.parametrize("M", [3, MAX_M])
def test_grid_wrap(M):
    states = _make(N_WRAP, M, (0, 64 * 40001, N_WRAP - 64), 100 + M)
    assert K.robust_agg_grid(N_WRAP) == 4096
    k = (M - 1) // 2
    out, sh, ct = _launch(states, k)
    _check(states, k, out, sh, ct)


def test_launch_geometry_independence(clients):
    for M, k in ((5, 1), (8, 3), (MAX_M, 2)):
        states = clients[:M]
        full, fsh, _ = _launch(states, k)
        for a, b in ((0, 1024), (1028, 2056), (2052, N), (4, 8)):
            out, sh, ct = _launch([s[a:b] for s in states], k)
            assert torch.equal(out.view(torch.int32), full[a:b].view(torch.int32)), (M, k, a, b)
            assert torch.equal(sh.view(torch.int16), fsh[a:b].view(torch.int16)), (M, k, a, b)
            assert int(_sums(ct)[:M].sum()) == 2 * k * (b - a)


@pytest.mark.parametrize("M,k", [(2, 0), (5, 2), (MAX_M, 7)])
def test_nothing_outside_the_buffers_is_written(M, k, clients):
    """out, shadow and counts sit between 64-element canaries; counts starts as garbage and every
    entry of every block row is overwritten, columns >= M with 0; the sources are not written."""
    C = 64
    states = [s.clone() for s in clients[:M]]
    obig = torch.full((N + 2 * C,), 1234.5, device=DEV)
    sbig = torch.full((N + 2 * C,), 7.0, dtype=torch.bfloat16, device=DEV)
    grid = K.robust_agg_grid(N)
    cbig = torch.full((COLS * grid + 2 * C,), -77, dtype=torch.int32, device=DEV)
    out, sh, ct = obig[C:C + N], sbig[C:C + N], cbig[C:C + COLS * grid]
    K.robust_agg(states, k, out, sh, ct)
    torch.cuda.synchronize()
    for can in (obig[:C], obig[C + N:]):
        assert torch.equal(can, torch.full_like(can, 1234.5))
    for can in (sbig[:C], sbig[C + N:]):
        assert torch.equal(can, torch.full_like(can, 7.0))
    for can in (cbig[:C], cbig[C + COLS * grid:]):
        assert torch.equal(can, torch.full_like(can, -77))
    rows = ct.view(grid, COLS)
    assert bool((rows >= 0).all())                       # (no entry keeps its garbage)
    assert not rows[:, M:MAX_M].any()
    assert rows[:, :M].sum(dim=1).tolist() == [2 * k * 1024] * 3 + [2 * k * (N - 3 * 1024)]
    _check(states, k, out, sh, ct)
    for s, c in zip(states, clients):
        assert torch.equal(s, c)


def test_determinism(clients):
    for M, k in ((4, 1), (MAX_M, 7)):
        a = _launch(clients[:M], k)
        b = _launch(clients[:M], k)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        assert torch.equal(a[1].view(torch.int16), b[1].view(torch.int16)) and torch.equal(a[2], b[2])
        # without the optional outputs: the same aggregate
        c = _launch(clients[:M], k, shadow=False, counts=False)
        assert torch.equal(a[0].view(torch.int32), c[0].view(torch.int32))


def test_adversarial_values(clients):
    """M = 5: one client all +NaN, one all -inf, one with -0 where the others hold +0.  k = 2 (the
    median) ignores them.  At k = 1 column 16 is the specification's ``nonfinite``: with +NaN at the
    top and -inf at the bottom of the order one of each end is trimmed and it is 0; with the NaN's
    sign bit set both sit at the bottom, only -NaN is trimmed, the -inf comes through and is counted."""
    states = [s.clone() for s in clients[:5]]
    states[1].fill_(float("nan"))
    assert not bool(torch.signbit(states[1]).any())
    states[3].fill_(float("-inf"))
    for p in PADS:
        states[0][p:p + 64] = -0.0
    out, sh, ct = _launch(states, 2)
    want, trimmed, nonfinite = _check(states, 2, out, sh, ct)
    assert nonfinite == 0 and bool(torch.isfinite(out).all()) and int(_sums(ct)[MAX_M]) == 0
    assert int(trimmed[1]) == N and int(trimmed[3]) == N
    out, sh, ct = _launch(states, 1)
    want, trimmed, nonfinite = _check(states, 1, out, sh, ct)
    assert int(_sums(ct)[MAX_M]) == nonfinite == 0
    # -NaN sorts below -inf: k = 1 trims it and keeps the -inf
    states[1] = -states[1]
    assert bool(torch.signbit(states[1]).all())
    out, sh, ct = _launch(states, 1)
    want, trimmed, nonfinite = _check(states, 1, out, sh, ct)
    assert nonfinite == N > 0 and int(_sums(ct)[MAX_M]) == nonfinite and int(trimmed[1]) == N
    # -0 sorts below +0
    z = [torch.zeros(N, device=DEV), -torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)]
    out, sh, ct = _launch(z, 1)
    assert not out.view(torch.int32).any() and _sums(ct)[:3].tolist() == [0, N, N]


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
def test_robust_aggregate_on_a_model_arena(with_server):
    """``robust_aggregate_`` of 3 perturbed copies (one of them scaled by -4) on the default DistilBERT
    arena: the master is the specification's aggregate (or, with a server optimizer, the fp32 chain's
    step on it with inv = 1), the shadow the kernel wrote is the shadow a refresh would write, the pads
    stay +0, the liar is the most-trimmed slot, and a graphed training step runs on the result."""
    model = DDoSClassifier(device=DEV, impl="hip", seed=3)
    A = model.arena
    x0 = A.master.clone()
    live = torch.zeros(A.numel, dtype=torch.bool, device=DEV)
    for name in A.names():
        off, shape = A.offsets[name]
        live[off:off + math.prod(shape)] = True
    assert int((~live).sum()) > 0
    g = torch.Generator(device=DEV).manual_seed(5)
    states = [x0 + 1e-3 * torch.randn(A.numel, device=DEV, generator=g) * live for _ in range(3)]
    states[1] = states[1] * -4.0
    server = so.ServerOptimizer(model, "adam", lr=0.01) if with_server else None
    rep = rb.robust_aggregate_(model, states, 1, server)
    torch.cuda.synchronize()
    agg, trimmed, nonfinite = rb.torch_robust_(states, 1)
    assert rep["trimmed"] == trimmed.tolist() and rep["nonfinite"] == nonfinite == 0
    assert rep["k"] == 1 and rep["clients"] == 3 and rep["trimmed_share"] == [t / A.numel for t in rep["trimmed"]]
    assert rb.most_trimmed(rep)[0] == 1 and rep["trimmed_share"][1] > 0.9
    if with_server:
        x, m = x0.clone(), torch.zeros_like(x0)
        v = torch.full_like(x0, so.f32(server.tau * server.tau))
        so.torch_chain_("adam", agg, x, m, v, 1.0, server.lr, server.b1, server.b2, server.tau)
        # The robust aggregate fed to both is the same bits.  The server kernel and the chain each round
        # x' = x + step once (half an ulp of x' each, <= 2^-24 max|x| apiece) and their steps (<= 0.01)
        # differ by a few roundings of sqrt / divide (a few 2^-24 * 0.01): together below 2^-23 max|x|
        # + 1e-9; the bound leaves a factor of two (max|x| is ~1: the LayerNorm weights).
        assert float((A.master.double() - x.double()).abs().max()) <= 4 * 2.0 ** -24 * float(x.abs().max())
        assert torch.equal(server.x, A.master) and server.rounds == 1
        assert float((A.master - x0).abs().max()) <= 0.01 * (1 + 1e-3)
    else:
        assert torch.equal(A.master.view(torch.int32), agg.view(torch.int32))
    assert torch.equal(A.shadow.view(torch.int16), A.master.to(torch.bfloat16).view(torch.int16))
    assert not A.master[~live].view(torch.int32).any()
    model.eval()
    ids, mask, labels, tokens = _batch(16, 128, seed=1)
    with torch.no_grad():
        first = model.forward(ids, mask).clone()
        model.sync_shadow(force=True)
        second = model.forward(ids, mask).clone()
    assert torch.isfinite(first).all() and torch.equal(first, second)
    model.train()
    opt = ArenaAdam(model, lr=1e-3)
    opt.reset_state()
    st = GraphedTrainStep(make_step_fn(model, opt), warmup=1, bucket=model.packed_rows)
    before = A.master.clone()
    losses = [float(st(ids, mask, labels, tokens)) for _ in range(3)]
    torch.cuda.synchronize()
    assert st.failed is None and len(st.graphs) >= 1 and all(math.isfinite(v) for v in losses)
    assert not torch.equal(A.master, before)


def test_one_client_and_too_many():
    model = DDoSClassifier(device=DEV, impl="hip", seed=3)
    A = model.arena
    s = A.master * 0.5
    rep = rb.robust_aggregate_(model, [s], 0)
    assert torch.equal(A.master, s) and rep["trimmed"] == [0] and rep["clients"] == 1
    assert torch.equal(A.shadow.view(torch.int16), s.to(torch.bfloat16).view(torch.int16))
    with pytest.raises(ValueError, match="at most 16"):
        rb.robust_aggregate_(model, [s] * 17, 0)
    bad = [s, torch.full_like(s, float("nan")), torch.full_like(s, float("nan"))]
    with pytest.raises(RuntimeError, match="non-finite"):
        rb.robust_aggregate_(model, bad, 1)


def test_refusals():
    """The binding rejects each invalid call before any launch: the buffers keep their contents."""
    n = 2048
    mk = lambda k=n, dt=torch.float32: torch.ones(k, dtype=dt, device=DEV)  # noqa: E731
    srcs = [mk(), mk(), mk()]
    out, sh = mk(), mk(dt=torch.bfloat16)
    ct = torch.ones(COLS * K.robust_agg_grid(n), dtype=torch.int32, device=DEV)
    ext = K.ext()
    ok = dict(srcs=srcs, k=1, out=out, shadow=sh, counts=ct)

    def bad(**kw):
        with pytest.raises(RuntimeError):
            ext.robust_agg(**dict(ok, **kw))

    bad(srcs=[mk()])                                   # M = 1
    bad(srcs=[mk() for _ in range(17)])                # M = 17
    bad(k=2)                                           # 2k >= M
    bad(srcs=[mk(), mk()], k=1)
    bad(k=-1)
    bad(srcs=[mk(n - 2)] * 3, out=mk(n - 2), shadow=None, counts=None)  # numel % 4
    bad(srcs=[mk(), mk(dt=torch.float64), mk()])       # dtype
    bad(out=mk(dt=torch.bfloat16))
    bad(shadow=mk())                                   # fp32 shadow
    bad(counts=ct.float())
    bad(srcs=[mk(), mk(2 * n)[::2], mk()])             # not contiguous
    bad(srcs=[mk(), mk(n - 4), mk()])                  # sizes
    bad(out=mk(n + 4))
    bad(shadow=mk(n - 4, torch.bfloat16))
    bad(counts=ct[:-1])                                # short counts
    bad(srcs=[mk(), mk().cpu(), mk()])                 # another device
    bad(out=srcs[1])                                   # out is a source
    big = mk(2 * n)
    bad(srcs=[mk(), big[:n], mk()], out=big[n // 2:n // 2 + n])  # out overlaps a source
    torch.cuda.synchronize()
    assert all(torch.equal(t, torch.ones_like(t)) for t in srcs + [out, sh, ct])
    K.robust_agg([mk(), big[:n], mk()], 1, big[n:], sh, ct)      # beside a source: accepted
    torch.cuda.synchronize()
    assert torch.equal(big[n:], torch.ones(n, device=DEV)) and _sums(ct)[:3].tolist() == [n, 0, n]
