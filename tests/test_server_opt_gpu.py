"""The fused FedOpt server step on the GPU (csrc/kernels/head_optim.hip ``server_opt_kernel`` through
``ops.kernels.server_opt`` and ``parallel.server_opt.ServerOptimizer``): against the fp32 torch chain
and an fp64 evaluation of the same fp32 inputs, output consistency (master / x / bf16 shadow / pads),
launch-geometry independence, the avgm launch without v, the deterministic per-block statistics, the
step on a real model arena, and the binding's refusals.

The vector has 4096 * 1024 + 4 * 257 floats: the 4 096-block grid-stride loop wraps once and the
wrapped pass fills one block and one float4 of the next.  Sum weight 3 -> inv = float32(1 / 3)."""
import math

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, GraphedTrainStep, make_step_fn)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.fed import runner
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as K
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.parallel import (
    server_opt as so)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 4096 * 1024 + 4 * 257
NCLIENTS, ROUNDS = 3, 3
KINDS = ("avgm", "adagrad", "adam", "yogi")
PADS = (0, 64 * 1000, 64 * 40001, N - 4 * 257 - 60, N - 64)  # 64-element alignment pads (+0 in every input)
B1, B2, TAU = so.f32(0.9), so.f32(0.99), so.f32(1e-3)
INV = so.f32(1.0 / NCLIENTS)


def _eta(kind):
    return so.f32(1.0 if kind == "avgm" else 0.01)


def _pad_mask():
    mask = torch.zeros(N, dtype=torch.bool, device=DEV)
    for p in PADS:
        mask[p:p + 64] = True
    return mask


@pytest.fixture(scope="module")
def inputs():
    """x ~ 0.05 N(0, 1) and the three rounds' client noise ~ 1e-3 N(0, 1), zero on the pads; computed
    once and never written."""
    g = torch.Generator(device=DEV).manual_seed(11)
    pad = _pad_mask()
    x0 = (0.05 * torch.randn(N, device=DEV, generator=g)).masked_fill_(pad, 0.0)
    noise = [(1e-3 * torch.randn(N, device=DEV, generator=g)).masked_fill_(pad, 0.0) for _ in range(ROUNDS)]
    return x0, noise, ~pad


def _v0(kind):
    return None if kind == "avgm" else torch.full((N,), so.f32(TAU * TAU), device=DEV)


def _launch(kind, s, x, m, v, shadow, stats=None, sl=slice(None)):
    K.server_opt(s[sl], x[sl], m[sl], None if v is None else v[sl], None if shadow is None else shadow[sl], kind,
                 INV, _eta(kind), B1, B2, TAU, stats)


@pytest.fixture(scope="module")
def rounds(inputs):
    """Three rounds per kind, three ways from the same fp32 inputs: (a) the kernel, (b) the fp32 torch
    chain on the device, (c) the chain in fp64 with the fp32 scalars (inv = float32(1 / 3), the fp32
    hyper-parameters and their fp32 1 - b).  Round r's sum is 3 (x_a + noise_r) with x_a the kernel's
    current x.  Per kind and round: every state of the three, the kernel's outputs and statistics."""
    x0, noise, _ = inputs
    out = {}
    grid = K.server_opt_grid(N)
    for kind in KINDS:
        eta = _eta(kind)
        a = [x0.clone(), torch.zeros(N, device=DEV), _v0(kind)]
        b = [t if t is None else t.clone() for t in a]
        c = [t if t is None else t.double() for t in a]
        recs = []
        for r in range(ROUNDS):
            s = NCLIENTS * (a[0] + noise[r])
            master, shadow = s.clone(), torch.zeros(N, dtype=torch.bfloat16, device=DEV)
            stats = torch.full((2 * grid,), float("nan"), device=DEV)
            _launch(kind, master, a[0], a[1], a[2], shadow, stats)
            so.torch_chain_(kind, s, b[0], b[1], b[2], INV, eta, B1, B2, TAU)
            d64, dx64 = so.torch_chain_(kind, s.double(), c[0], c[1], c[2], INV, eta, B1, B2, TAU)
            recs.append({"s": s, "master": master, "shadow": shadow, "stats": stats,
                         "a": [t if t is None else t.clone() for t in a],
                         "b": [t if t is None else t.clone() for t in b],
                         "c": [t if t is None else t.clone() for t in c],
                         "sum_d2": float(d64.square().sum()), "sum_dx2": float(dx64.square().sum())})
        out[kind] = recs
    torch.cuda.synchronize()
    return out


def _ulp32(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23)


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_against_fp32_chain_and_fp64(kind, rounds, inputs):
    """max|kernel - fp64| <= 2 max(max|fp32 chain - fp64|, ulp32(max|x|)) for x', m and v after each of
    3 rounds: the kernel rounds every operation once, like the chain (2x: a contracted or reordered
    operation would change single roundings, not the error's order)."""
    names = ("x", "m") if kind == "avgm" else ("x", "m", "v")
    for r, rec in enumerate(rounds[kind]):
        floor = _ulp32(float(rec["c"][0].abs().max()))
        for i, name in enumerate(names):
            ac = float((rec["a"][i].double() - rec["c"][i]).abs().max())
            bc = float((rec["b"][i].double() - rec["c"][i]).abs().max())
            print(f"server_opt {kind} round {r + 1} {name}: max|kernel - fp64| {ac:.3e}  "
                  f"max|torch fp32 - fp64| {bc:.3e}  ulp32(max|x|) {floor:.3e}  "
                  f"kernel == torch fp32 bitwise: {torch.equal(rec['a'][i], rec['b'][i])}")
            assert ac <= 2.0 * max(bc, floor), (kind, r, name, ac, bc, floor)
        prev = inputs[0] if r == 0 else rounds[kind][r - 1]["a"][0]
        assert not torch.equal(rec["a"][0], prev)  # (the step did move x)


@pytest.mark.parametrize("kind", KINDS)
def test_outputs_are_consistent(kind, rounds, inputs):
    pad = ~inputs[2]
    v_pad = torch.tensor(so.f32(TAU * TAU), device=DEV)
    for rec in rounds[kind]:
        x, m, v = rec["a"]
        assert torch.equal(rec["master"], x)
        assert torch.equal(rec["shadow"], x.to(torch.bfloat16))
        assert torch.equal(rec["shadow"].view(torch.int16), x.to(torch.bfloat16).view(torch.int16))
        for t in (rec["master"], x, m):  # exactly +0: no bit set
            assert not t[pad].view(torch.int32).any()
        assert not rec["shadow"][pad].view(torch.int16).any()
        assert torch.isfinite(x).all() and torch.isfinite(m).all()
        if v is not None:
            # d = 0 on a pad: adam's v decays by b2 a round, adagrad's and yogi's stays tau^2
            if kind == "adam":
                v_pad = v_pad * B2
            assert torch.isfinite(v).all() and (v >= 0).all()
            assert torch.equal(v[pad], v_pad.expand(int(pad.sum())))


@pytest.mark.parametrize("kind", KINDS)
def test_launch_geometry_independence(kind, rounds, inputs):
    """One launch over the vector == launches over three unequal 4-aligned slices, bitwise (a short
    one of a single block, one whose grid-stride loop does not wrap, one that starts mid-block)."""
    x0 = inputs[0]
    rec = rounds[kind][0]
    master, x, m, v = rec["s"].clone(), x0.clone(), torch.zeros(N, device=DEV), _v0(kind)
    shadow = torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    for sl in (slice(0, 4 * 57), slice(4 * 57, 4 * 57 + 4 * 300_001), slice(4 * 57 + 4 * 300_001, N)):
        _launch(kind, master, x, m, v, shadow, None, sl)
    assert torch.equal(master, rec["master"]) and torch.equal(x, rec["a"][0]) and torch.equal(m, rec["a"][1])
    assert torch.equal(shadow.view(torch.int16), rec["shadow"].view(torch.int16))
    if v is not None:
        assert torch.equal(v, rec["a"][2])


@pytest.mark.parametrize("kind", ["avgm", "adam"])
def test_nothing_outside_the_buffers_is_written(kind, rounds, inputs):
    """Every buffer sits between 64-float canaries in one allocation, the tail of the last block
    included; avgm runs with v=None and leaves the NaN-filled buffer where another kind's v would lie
    (right behind m) untouched."""
    x0 = inputs[0]
    rec = rounds[kind][0]
    C = 64
    big = torch.full((4 * N + 5 * C,), 1234.5, device=DEV)
    offs = [C + i * (N + C) for i in range(4)]
    master, x, m, vbuf = (big[o:o + N] for o in offs)
    master.copy_(rec["s"])
    x.copy_(x0)
    m.zero_()
    if kind == "avgm":
        vbuf.fill_(float("nan"))
    else:
        vbuf.copy_(_v0(kind))
    sbig = torch.full((N + 2 * C,), 7.0, dtype=torch.bfloat16, device=DEV)
    shadow = sbig[C:C + N]
    grid = K.server_opt_grid(N)
    stbig = torch.full((2 * grid + 2 * C,), -3.0, device=DEV)
    _launch(kind, master, x, m, None if kind == "avgm" else vbuf, shadow, stbig[C:C + 2 * grid])
    torch.cuda.synchronize()
    for i in range(5):
        can = big[i * (N + C):i * (N + C) + C]
        assert torch.equal(can, torch.full_like(can, 1234.5)), i
    for can in (sbig[:C], sbig[C + N:]):
        assert torch.equal(can, torch.full_like(can, 7.0))
    for can in (stbig[:C], stbig[C + 2 * grid:]):
        assert torch.equal(can, torch.full_like(can, -3.0))
    assert torch.equal(x, rec["a"][0]) and torch.equal(m, rec["a"][1]) and torch.equal(master, x)
    assert torch.equal(stbig[C:C + 2 * grid], rec["stats"])
    if kind == "avgm":
        assert torch.isnan(vbuf).all()
        assert torch.equal(vbuf.view(torch.int32), torch.full_like(vbuf, float("nan")).view(torch.int32))
    else:
        assert torch.equal(vbuf, rec["a"][2])


@pytest.mark.parametrize("kind", KINDS)
def test_stats(kind, rounds, inputs):
    """The per-block partials, summed in fp64, are sum (avg - x)^2 and sum (x' - x)^2 of the fp64
    evaluation to a relative 1e-5 (a lane adds at most 8 squares, a block 2 048, in fp32: that bound
    is loose by orders of magnitude), every block writes its pair, and a second run gives the same
    bits."""
    grid = K.server_opt_grid(N)
    assert grid == 4096
    for rec in rounds[kind]:
        st = rec["stats"]
        assert st.numel() == 2 * grid and torch.isfinite(st).all() and (st >= 0).all()
        got = st.view(-1, 2).sum(dim=0, dtype=torch.float64).tolist()
        print(f"server_opt {kind}: sum d^2 {got[0]:.9e} (fp64 {rec['sum_d2']:.9e})  "
              f"sum (x' - x)^2 {got[1]:.9e} (fp64 {rec['sum_dx2']:.9e})")
        assert abs(got[0] - rec["sum_d2"]) <= 1e-5 * rec["sum_d2"]
        assert abs(got[1] - rec["sum_dx2"]) <= 1e-5 * rec["sum_dx2"]
    rec = rounds[kind][0]
    master, x, m, v = rec["s"].clone(), inputs[0].clone(), torch.zeros(N, device=DEV), _v0(kind)
    again = torch.zeros(2 * grid, device=DEV)
    _launch(kind, master, x, m, v, None, again)
    assert torch.equal(again, rec["stats"]) and torch.equal(x, rec["a"][0])  # (no shadow: same x')


def _batch(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(S // 3, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids = ids * mask
    ids[:, 0] = 101
    labels = torch.randint(0, 2, (B,), generator=g)
    return ids.cuda(), mask.cuda(), labels.cuda(), int(lens.sum())


def test_server_step_on_a_model_arena():
    """``_average_masters(model, [a, b], server)`` on the default DistilBERT arena: the shadow the
    kernel wrote is the shadow a refresh would write (same logits before and after
    ``sync_shadow(force=True)``), the server's x is the master, the pads stay +0, the norms are those of
    the fp64 evaluation, and a graphed training step runs on the result and moves the weights."""
    model = DDoSClassifier(device=DEV, impl="hip", seed=3)
    A = model.arena
    x0 = A.master.clone()
    live = torch.zeros(A.numel, dtype=torch.bool, device=DEV)
    for name in A.names():
        off, shape = A.offsets[name]
        live[off:off + math.prod(shape)] = True
    assert not x0[~live].view(torch.int32).any() and int((~live).sum()) > 0
    g = torch.Generator(device=DEV).manual_seed(5)
    a = x0 + 1e-3 * torch.randn(A.numel, device=DEV, generator=g) * live
    b = x0 + 1e-3 * torch.randn(A.numel, device=DEV, generator=g) * live
    server = so.ServerOptimizer(model, "adam", lr=0.01)
    assert server.x.device == A.master.device and torch.equal(server.x, x0)
    norms = runner._average_masters(model, [a, b], server)
    torch.cuda.synchronize()
    assert torch.equal(server.x, A.master) and not torch.equal(A.master, x0)
    assert torch.equal(A.shadow.view(torch.int16), A.master.to(torch.bfloat16).view(torch.int16))
    for t in (A.master, server.x, server.m):
        assert not t[~live].view(torch.int32).any()
    d = ((a + b).double() * so.f32(0.5) - x0.double())
    assert abs(norms["delta_l2"] - float(d.norm())) <= 1e-5 * float(d.norm())
    step = float((A.master.double() - x0.double()).norm())
    assert abs(norms["step_l2"] - step) <= 1e-5 * step and step > 0
    # round 1 of FedAdam moves no weight by more than eta (1 - b1) / sqrt(1 - b2) = eta (plus rounding)
    assert float((A.master - x0).abs().max()) <= 0.01 * (1 + 1e-3)
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
    assert not torch.equal(A.master, before) and torch.equal(server.x, before)


def test_refusals():
    """The binding rejects each invalid call before any launch: the buffers keep their contents."""
    n = 2048
    mk = lambda k=n, dt=torch.float32: torch.ones(k, dtype=dt, device=DEV)  # noqa: E731
    ms, x, m, v, sh = mk(), mk(), mk(), mk(), mk(dt=torch.bfloat16)
    st = torch.ones(2 * K.server_opt_grid(n), device=DEV)
    ext = K.ext()
    ok = dict(master=ms, x=x, m=m, v=v, shadow=sh, kind=2, inv=0.5, eta=0.01, b1=0.9, b2=0.99, tau=1e-3, stats=st)

    def bad(**kw):
        with pytest.raises(RuntimeError):
            ext.server_opt(**dict(ok, **kw))

    bad(x=mk(n - 4))
    bad(m=mk(n - 4))
    bad(v=mk(n - 4))
    bad(shadow=mk(n - 4, torch.bfloat16))
    bad(v=None)                      # adam without v
    bad(kind=0)                      # avgm with v
    bad(kind=4)
    bad(kind=-1)
    bad(x=mk(dt=torch.float64))
    bad(m=mk(dt=torch.bfloat16))
    bad(shadow=mk())                 # fp32 shadow
    bad(stats=st.double())
    bad(stats=st[:-1])               # short stats
    bad(x=mk(2 * n)[::2])            # not contiguous
    bad(x=mk().cpu())                # another device
    bad(master=mk(n - 2), x=mk(n - 2), m=mk(n - 2), v=mk(n - 2), shadow=None, stats=None)  # numel % 4
    for name in ("eta", "tau", "inv"):
        for val in (float("nan"), float("inf"), 0.0, -1.0):
            bad(**{name: val})
    for name in ("b1", "b2"):
        for val in (float("nan"), 1.0, -0.1):
            bad(**{name: val})
    with pytest.raises(ValueError):
        K.server_opt(ms, x, m, v, sh, "sgd", 0.5, 0.01, 0.9, 0.99, 1e-3, st)
    torch.cuda.synchronize()
    for t in (ms, x, m, v, st):
        assert torch.equal(t, torch.ones_like(t))
    assert torch.equal(sh, torch.ones_like(sh))
    ext.server_opt(**ok)             # and the valid call runs
    torch.cuda.synchronize()
    assert not torch.equal(x, torch.ones_like(x)) and torch.equal(ms, x)
