"""The secure-aggregation kernels on the GPU (csrc/kernels/secagg.hip through ``ops.kernels.secagg_*`` and
``parallel.secagg.SecureAggregator``): the generator bit for bit against the host mirror and the RFC
8439 known answer, the mask pass bit for bit against the specification (P = 0) and against ``q`` plus
the signed device streams (P = 1, 2, 7, 15), the unmask pass bit for bit, the bit balance of a masked
zero update, a slice with ``first_block``, launch-geometry independence, canaries, run-to-run
determinism, a real model arena, the binding's refusals, and the public-key gather through ``NativeComm``
(one rank here; ``setup_keys`` and a masked exchange over RCCL where two GPUs are visible).

Everything but the two norms is integer arithmetic or a chain of single fp32 operations, so every
comparison but theirs is bitwise.  Shapes: one block (16), 2048, and the smallest multiple of 16 above
one full sweep of the capped grid (2048 blocks x 1024 elements), where the grid-stride loop wraps with
a ragged last sweep."""
import math

import numpy as np
import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, GraphedTrainStep, make_step_fn)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as K
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.parallel import (
    secagg as sa)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N1 = 16
N = 2048
GRID_CAP = 2048
N_WRAP = GRID_CAP * 1024 + 16     # one full sweep of 2048 x 256 lanes, then 8 lanes (4 of them the check block)
F = 24
RFC_KEY = np.frombuffer(bytes(range(32)), dtype="<u4")
RFC_NONCE = (0x09000000, 0x4A000000, 0)
RFC_WORDS = [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
             0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]


def _i32(t):
    return t.view(torch.int32)


def _keys(P, seed=11):
    """[P, 8] key words: on the host (uint32) and on the device (int32)."""
    k = np.random.default_rng(seed).integers(0, 1 << 32, size=(P, 8), dtype=np.uint64).astype(np.uint32)
    return k, torch.from_numpy(k.view(np.int32).copy()).reshape(P, 8).to(DEV)


def _make(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    anchor = 0.05 * torch.randn(n, device=DEV, generator=g)
    w = anchor + 1e-3 * torch.randn(n, device=DEV, generator=g) * torch.rand(n, device=DEV, generator=g)
    w[:16] = 0.0                         # a pad: +0 in w and anchor
    anchor[:16] = 0.0
    return w, anchor


@pytest.fixture(scope="module")
def small():
    t = _make(N, 17)
    return t, tuple(x.cpu() for x in t)


@pytest.fixture(scope="module")
def wrap():
    t = _make(N_WRAP, 23)
    return t, tuple(x.cpu() for x in t)


def _stream(n, key_dev, nonce, rounds=20, first_block=0):
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    K.secagg_stream(out, key_dev, nonce, rounds, first_block)
    return out


def _mask(w, a, keys_dev, signs=0, frac_bits=F, rounds=20, round=0, first_block=0):
    n = w.numel()
    payload = torch.full((K.secagg_words(n),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    partial = torch.full((4 * K.secagg_grid(n),), float("nan"), dtype=torch.float64, device=DEV)
    stats = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    K.secagg_mask(w, a, keys_dev, signs, payload, partial, stats, frac_bits, rounds, round, first_block)
    return payload, stats, partial


def test_grid_and_words():
    assert K.SECAGG_MAX_CLIENTS == sa.MAX_CLIENTS == 16
    assert K.secagg_grid(N1) == 1 and K.secagg_grid(N) == 3 and K.secagg_grid(N_WRAP - 16) == GRID_CAP
    assert K.secagg_grid(N_WRAP) == GRID_CAP and K.secagg_grid(1 << 26) == GRID_CAP
    for n in (N1, N, N_WRAP):
        assert K.secagg_words(n) == sa.secagg_words(n) == n + 16


@pytest.mark.parametrize("rounds", [8, 12, 20])
def test_stream_equals_the_host_mirror(rounds):
    kh, kd = _keys(1, seed=rounds)
    nonce = (7, 0xDEADBEEF, 0xFFFFFFFF)
    for n in (N1, N):
        for fb in (0, 1, (1 << 32) - n // 16 - 1, (1 << 32) - n // 16):
            got = _stream(n, kd[0], nonce, rounds, fb)
            want = sa.stream_words(kh[0], nonce, n, fb, rounds)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want), (n, fb)
    if rounds == 8:                        # the grid-stride loop wraps (the mirror is cheapest at 8 rounds)
        got = _stream(N_WRAP, kd[0], nonce, rounds, 5)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), sa.stream_words(kh[0], nonce, N_WRAP, 5, rounds))


def test_stream_rfc_8439_known_answer():
    kd = torch.from_numpy(RFC_KEY.view(np.int32).copy()).to(DEV)
    got = _stream(16, kd, RFC_NONCE, 20, 1).cpu().numpy().view(np.uint32)
    assert [int(got[e]) for e in range(16)] == [RFC_WORDS[sa.WORD_ORDER[e]] for e in range(16)]
    assert sorted(sa.WORD_ORDER) == list(range(16)) and sa.WORD_ORDER[1] == 4 and sa.WORD_ORDER[4] == 1


def _crafted():
    """(w, anchor, expected q, expected clamped, expected bad) at f = 24: anchor 0, so d = w."""
    u = 2.0 ** -F
    below = float(np.nextafter(np.float32(8.0), np.float32(0.0)))      # one ulp below 2^27 * 2^-f
    rows = [(0.0, 0), (-0.0, 0), (0.5 * u, 0), (1.5 * u, 2), (2.5 * u, 2), (-0.5 * u, 0), (-1.5 * u, -2),
            (below, (1 << 27) - 8), (-below, -((1 << 27) - 8)), (8.0, "c+"), (-8.0, "c-"), (3e38, "c+"), (-1e38, "c-"),
            (float("inf"), "b"), (float("-inf"), "b"), (float("nan"), "b"), (1e-40, 0), (-1e-40, 0), (1.0, 1 << 24),
            (-0.25, -(1 << 22))]
    n = 32
    w, a = torch.zeros(n), torch.zeros(n)
    q = [0] * n
    for i, (v, e) in enumerate(rows):
        w[i] = v
        q[i] = sa.QMAX if e == "c+" else -sa.QMAX if e == "c-" else 0 if e == "b" else e
    w[30], a[30] = 3e38, -3e38                                          # w - anchor overflows: d = inf, bad
    clamped = sum(1 for _, e in rows if e in ("c+", "c-"))
    bad = sum(1 for _, e in rows if e == "b") + 1
    return w, a, torch.tensor(q, dtype=torch.int32), clamped, bad


def test_mask_without_partners_is_the_quantizer(small, wrap):
    _, k0 = _keys(0)
    one = torch.ones(16, dtype=torch.int32)
    for (w, a), (wc, ac) in (small, wrap, ((small[0][0][:N1], small[0][1][:N1]), (small[1][0][:N1], small[1][1][:N1]))):
        n = w.numel()
        payload, stats, _ = _mask(w, a, k0)
        q, rep = sa.torch_encode(wc, ac, F)
        assert torch.equal(payload[:n].cpu(), q) and torch.equal(payload[n:].cpu(), one)
        assert torch.equal(payload.cpu(), sa.torch_mask(q, np.zeros((0, 8)), 0))
        up, er, cl, bad = stats.tolist()
        assert cl == 0.0 and bad == 0.0 and rep["clamped"] == 0 and rep["bad_elems"] == 0
        assert abs(up - rep["update_l2"]) <= 2.0 ** -23 * up and abs(er - rep["error_l2"]) <= 2.0 ** -23 * er
        assert not payload[:16].any() if n > 16 else True               # the pad's code is 0
    # another fraction width
    (w, a), (wc, ac) = small
    for f in (8, 30):
        payload, stats, _ = _mask(w, a, k0, frac_bits=f)
        q, rep = sa.torch_encode(wc, ac, f)
        assert torch.equal(payload[:N].cpu(), q) and stats[2].item() == rep["clamped"]


def test_mask_crafted_vector():
    w, a, q_want, clamped, bad = _crafted()
    _, k0 = _keys(0)
    payload, stats, _ = _mask(w.to(DEV), a.to(DEV), k0)
    q, rep = sa.torch_encode(w, a, F)
    assert torch.equal(q, q_want) and rep["clamped"] == clamped and rep["bad_elems"] == bad   # the specification, by hand
    assert torch.equal(payload[:32].cpu(), q_want) and torch.equal(payload[32:].cpu(), torch.ones(16, dtype=torch.int32))
    up, er, cl, nb = stats.tolist()
    assert cl == float(clamped) and nb == float(bad)
    assert math.isfinite(up) and abs(up - rep["update_l2"]) <= 2.0 ** -23 * up
    assert abs(er - rep["error_l2"]) <= 2.0 ** -23 * er


@pytest.mark.parametrize("which", ["small", "wrap"])
def test_stats(which, request):
    """|d| and |d - float(q) 2^-f| against fp64.  The device squares in fp64 (exact for fp32 inputs) and
    adds n non-negative doubles in a fixed order; so does the reference, in another order: the two sums
    of squares agree within 2 n 2^-53, their roots within half that, and the fp32 roundings of two roots
    that close are at most one ulp apart.  The two counts are exact."""
    (w, a), _ = request.getfixturevalue(which)
    n = w.numel()
    w = w.clone()
    bad = [40, n - 7] + ([1234567] if n == N_WRAP else [])
    big = [100, n - 33]
    for k, i in enumerate(bad):
        w[i] = float("nan") if k % 2 == 0 else float("inf")
    for k, i in enumerate(big):
        w[i] = a[i] + (9.0 if k % 2 == 0 else -100.0)
    _, k0 = _keys(0)
    payload, stats, partial = _mask(w, a, k0)
    up, er, cl, nb = stats.tolist()
    assert cl == float(len(big)) and nb == float(len(bad))
    p = partial.view(-1, 4)
    assert bool(torch.isfinite(p).all()) and float(p[:, 2].sum()) == len(big) and float(p[:, 3].sum()) == len(bad)
    good = torch.ones(n, dtype=torch.bool, device=DEV)
    good[bad] = False
    d = (w - a)[good]
    back = payload[:n][good].to(torch.float32) * 2.0 ** -F
    e = d - back
    for got, S, ref in ((up, float(p[:, 0].sum()), d.double()), (er, float(p[:, 1].sum()), e.double())):
        want = float(ref.square().sum())
        rel = abs(S - want) / want
        print(f"secagg_mask n={n}: relative error of a sum of squares {rel:.3e} (bound {2 * n * 2.0 ** -53:.3e})")
        assert rel <= 2 * n * 2.0 ** -53
        r32 = torch.tensor(math.sqrt(want), dtype=torch.float64).to(torch.float32)
        ulp = abs(float(torch.nextafter(r32, torch.tensor(float("inf"))) - r32))
        assert abs(got - float(r32)) <= ulp and got == float(torch.tensor(got).float())


def _q_plus_streams(q_dev, n, kd, signs, rounds, round, first_block):
    """uint32(q) and the check block's ones plus the signed device streams, modulo 2^32 (int32)."""
    y = torch.cat([q_dev.to(torch.int64), torch.ones(16, dtype=torch.int64, device=DEV)])
    for p in range(kd.shape[0]):
        x = _stream(n + 16, kd[p], (round, 0, 0), rounds, first_block).to(torch.int64)
        y = y - x if (signs >> p) & 1 else y + x
    y = y & 0xFFFFFFFF
    return torch.where(y >= 1 << 31, y - (1 << 32), y).to(torch.int32)


@pytest.mark.parametrize("P", [1, 2, 7, 15])
def test_mask_is_q_plus_the_signed_streams(P, small, wrap):
    _, k0 = _keys(0)
    kh, kd = _keys(P, seed=100 + P)
    signs = 0b101101001110010 & ((1 << P) - 1)
    cases = [(small[0], 20, 3, 0), ((small[0][0][:N1], small[0][1][:N1]), 12, 0, (1 << 32) - 2),
             (wrap[0], 8 if P > 2 else 20, 9, 77)]
    for (w, a), rounds, rnd, fb in cases:
        n = w.numel()
        q = _mask(w, a, k0)[0][:n]
        payload, stats, _ = _mask(w, a, kd, signs, F, rounds, rnd, fb)
        assert torch.equal(payload, _q_plus_streams(q, n, kd, signs, rounds, rnd, fb)), (n, rounds)
        assert torch.equal(stats, _mask(w, a, k0)[1])                    # the masks do not touch the stats
    # ... and the host specification, at the small shapes
    (w, a), (wc, ac) = small
    q, _ = sa.torch_encode(wc, ac, F)
    payload, _, _ = _mask(w, a, kd, signs, F, 20, 3, 0)
    assert torch.equal(payload.cpu(), sa.torch_mask(q, kh, signs, 3, 20, 0))
    assert int((payload[:N].cpu() == q).sum()) <= N // 100              # a payload is not its plaintext


@pytest.fixture(scope="module")
def clients(small):
    """16 clients' updates at N against one anchor, with sums at +-16 (2^27 - 1) in six elements."""
    _, (_, ac) = small
    ws = []
    for c in range(16):
        g = torch.Generator().manual_seed(200 + c)
        w = ac + (1e-3 * (c + 1)) * torch.randn(N, generator=g)
        w[:16] = 0.0
        w[100:103] = ac[100:103] + 8.0 + c        # clamped high in every client
        w[200:203] = ac[200:203] - 9.0 - c        # clamped low
        ws.append(w)
    return ws


@pytest.mark.parametrize("M", [1, 2, 3, 8, 16])
def test_unmask_mean_equals_the_specification(M, small, clients):
    (_, a), (_, ac) = small
    agg = sa.SecureAggregator(F, 8, seed=5)
    agg.setup_keys(range(M), M)
    live = list(range(M))
    masked = [agg.mask_(clients[c], ac, c, 4, live) for c in live]
    plain = [sa.torch_mask(sa.torch_encode(clients[c], ac, F)[0], np.zeros((0, 8)), 0) for c in live]
    assert agg.last["clamped"] == 6 and agg.last["masked_with"] == M - 1
    want, wsh = torch.empty(N), torch.empty(N, dtype=torch.bfloat16)
    sa.torch_unmask_mean_(masked, ac, want, wsh, F)
    for ps in (masked, plain):                                         # equal to the unmasked quantized mean
        for shadow in (True, False):
            out = torch.full((N,), 7.0, device=DEV)
            sh = torch.full((N,), 7.0, dtype=torch.bfloat16, device=DEV) if shadow else None
            K.secagg_unmask_mean([p.to(DEV) for p in ps], a, out, sh, F)
            assert torch.equal(_i32(out.cpu()), _i32(want))
            if shadow:
                assert torch.equal(sh.cpu().view(torch.int16), wsh.view(torch.int16))
            assert not _i32(out[:16]).any()                            # the pad stays +0
    s = sum(p[:N].to(torch.int64) for p in plain)
    assert int(s[100]) == M * sa.QMAX and int(s[200]) == -M * sa.QMAX
    # the clamped elements moved by exactly +-(2^27 - 1) 2^-f (float(M qmax) rounds to M 2^27 for these M)
    assert torch.equal(want[100:103], ac[100:103] + (float(np.float32(M * sa.QMAX)) * 2.0 ** -F) * float(np.float32(1.0 / M)))


def test_unmask_mean_wrap(wrap):
    (w, a), (wc, ac) = wrap
    kh, kd = _keys(1, seed=9)
    p0, _, _ = _mask(w, a, kd, 0, F, 8, 2, 0)
    p1, _, _ = _mask(a.clone(), a, kd, 1, F, 8, 2, 0)                          # the partner sends a zero update
    out = torch.empty(N_WRAP, device=DEV)
    sh = torch.empty(N_WRAP, dtype=torch.bfloat16, device=DEV)
    assert torch.equal(sa.check_block_sum([p0, p1]).cpu(), torch.full((16,), 2, dtype=torch.int64))
    K.secagg_unmask_mean([p0, p1], a, out, sh, F)
    q, _ = sa.torch_encode(wc, ac, F)
    plain = sa.torch_mask(q, np.zeros((0, 8)), 0)
    zero = sa.torch_mask(torch.zeros_like(q), np.zeros((0, 8)), 0)
    want, wsh = torch.empty(N_WRAP), torch.empty(N_WRAP, dtype=torch.bfloat16)
    sa.torch_unmask_mean_([plain, zero], ac, want, wsh, F)
    assert torch.equal(_i32(out.cpu()), _i32(want)) and torch.equal(sh.cpu().view(torch.int16), wsh.view(torch.int16))


def test_bit_balance_of_a_masked_zero_update():
    """65,536 words of a zero update under one stream: every bit position is set in half of them, within
    5 sigma (sigma = sqrt(n) / 2 = 128)."""
    n = 1 << 16
    z = torch.zeros(n, device=DEV)
    z2 = torch.zeros(n, device=DEV)
    for rounds in (8, 20):
        _, kd = _keys(1, seed=rounds)
        payload, _, _ = _mask(z, z2, kd, 0, F, rounds, 1, 0)
        words = payload[:n].to(torch.int64) & 0xFFFFFFFF
        for b in range(32):
            ones = int(((words >> b) & 1).sum())
            assert abs(ones - n // 2) <= 5 * 128, (rounds, b, ones)


def test_a_slice_with_first_block_equals_the_range_of_the_whole(small):
    (w, a), _ = small
    _, kd = _keys(3, seed=4)
    whole, _, _ = _mask(w, a, kd, 0b010, F, 20, 6, 1000)
    for lo, hi in ((0, 512), (512, 1536), (2032, 2048), (16, 48)):
        part, _, _ = _mask(w[lo:hi], a[lo:hi], kd, 0b010, F, 20, 6, 1000 + lo // 16)
        assert torch.equal(part[:hi - lo], whole[lo:hi])
    part, _, _ = _mask(w[2032:2048], a[2032:2048], kd, 0b010, F, 20, 6, 1000 + 2032 // 16)
    assert torch.equal(part[16:], whole[N:])                           # the last slice's check block is the whole's
    other, _, _ = _mask(w[512:1536], a[512:1536], kd, 0b010, F, 20, 6, 0)
    assert not torch.equal(other[:1024], whole[512:1536])              # (another part of the stream)
    another, _, _ = _mask(w, a, kd, 0b010, F, 20, 7, 1000)
    assert int((another[:N] == whole[:N]).sum()) <= N // 100           # (another round: another stream)


def test_launch_geometry_independence(wrap):
    """A word depends on its global element alone: a range cut at a boundary that is no multiple of the
    block (or of the sweep) is computed by other lanes, blocks and sweeps, and is the same."""
    (w, a), _ = wrap
    _, kd = _keys(2, seed=8)
    whole, _, _ = _mask(w, a, kd, 0b01, F, 8, 1, 0)
    stream = _stream(N_WRAP, kd[0], (1, 0, 0), 8, 0)
    for lo, hi in ((16 * 37, 16 * 37 + 4096), (1024 * 2047 + 16 * 3, N_WRAP), (16, N_WRAP - 16)):
        part, _, _ = _mask(w[lo:hi], a[lo:hi], kd, 0b01, F, 8, 1, lo // 16)
        assert torch.equal(part[:hi - lo], whole[lo:hi])
        assert torch.equal(_stream(hi - lo, kd[0], (1, 0, 0), 8, lo // 16), stream[lo:hi])


def test_nothing_outside_the_buffers_is_written(small):
    """Every buffer sits between 64-element canaries; payload, partial, stats and the stream start as
    garbage and every entry is overwritten; w, the anchor and the keys are not written."""
    C = 64
    (w0, a0), _ = small
    words, grid = K.secagg_words(N), K.secagg_grid(N)
    kh, kd0 = _keys(2, seed=6)

    def framed(k, val, dt=torch.float32):
        big = torch.full((k + 2 * C,), val, dtype=dt, device=DEV)
        return big, big[C:C + k]

    wbig, w = framed(N, 1234.5)
    abig, a = framed(N, 99.0)
    kbig, kflat = framed(16, 0x33333333, torch.int32)
    pbig, p = framed(words, 0x5A5A5A5A, torch.int32)
    qbig, part = framed(4 * grid, -77.0, torch.float64)
    tbig, st = framed(4, -5.0, torch.float64)
    obig, out = framed(N, 55.0)
    sbig, sh = framed(N, 7.0, torch.bfloat16)
    gbig, so = framed(N, 0x77777777, torch.int32)
    w.copy_(w0)
    a.copy_(a0)
    kflat.copy_(kd0.reshape(-1))
    kd = kflat.view(2, 8)
    K.secagg_mask(w, a, kd, 0b10, p, part, st, F, 20, 1, 0)
    K.secagg_unmask_mean([p, p.clone()], a, out, sh, F)
    K.secagg_stream(so, kd[1], (1, 0, 0), 20, 0)
    torch.cuda.synchronize()
    for big, k, val in ((wbig, N, 1234.5), (abig, N, 99.0), (kbig, 16, 0x33333333), (pbig, words, 0x5A5A5A5A),
                        (qbig, 4 * grid, -77.0), (tbig, 4, -5.0), (obig, N, 55.0), (sbig, N, 7.0),
                        (gbig, N, 0x77777777)):
        for can in (big[:C], big[C + k:]):
            assert torch.equal(can, torch.full_like(can, val))
    assert torch.equal(w, w0) and torch.equal(a, a0) and torch.equal(kd, kd0)
    assert bool((part >= 0).all()) and float(st[0]) > 0 and float(st[3]) == 0.0      # (no entry keeps its garbage)
    q, _ = sa.torch_encode(w0.cpu(), a0.cpu(), F)
    assert torch.equal(p.cpu(), sa.torch_mask(q, kh, 0b10, 1, 20, 0))
    assert np.array_equal(so.cpu().numpy().view(np.uint32), sa.stream_words(kh[1], (1, 0, 0), N, 0, 20))
    assert torch.equal(sh.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)) and bool(torch.isfinite(out).all())


def test_run_to_run_determinism(wrap):
    (w, a), _ = wrap
    _, kd = _keys(3, seed=2)
    first = _mask(w, a, kd, 0b110, F, 12, 2, 3)
    again = _mask(w, a, kd, 0b110, F, 12, 2, 3)
    assert torch.equal(first[0], again[0])
    assert torch.equal(first[1].view(torch.int64), again[1].view(torch.int64))
    assert torch.equal(first[2].view(torch.int64), again[2].view(torch.int64))
    outs = []
    for _ in range(2):
        out = torch.empty(N_WRAP, device=DEV)
        K.secagg_unmask_mean([first[0], again[0], first[0]], a, out, None, F)
        outs.append(out)
    assert torch.equal(_i32(outs[0]), _i32(outs[1]))


def test_public_keys_through_the_native_communicator():
    """The public-key gather through a real ``NativeComm`` (one rank, this GPU): the binding's dtype check
    takes the 8 int32 words the key travels as -- it refuses a uint8 tensor -- and the bytes come back as
    they went."""
    from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.parallel.rccl import (
        NativeComm)
    c = NativeComm(rank=0, world_size=1)
    try:
        pk = sa.public_key(sa.private_key(7, 0))
        assert sa.gather_public_keys(pk, 1, c, DEV) == [pk]
        with pytest.raises(RuntimeError, match="unsupported dtype"):
            c.all_gather(torch.zeros(32, dtype=torch.uint8, device=DEV))
    finally:
        c.close()


def _two_gpu_keys_worker(rank, world, port, outdir):
    import os
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    os.environ.pop("FEDDDOS_BACKEND", None)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from importlib import import_module
    pkg = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"
    comm = import_module(f"{pkg}.parallel.comm")
    di = comm.init_distributed(timeout_s=120)
    c = import_module(f"{pkg}.parallel.rccl").NativeComm()
    s = sa.SecureAggregator(F, 8)
    s.setup_keys(rank, world, comm=c, device=di.device)
    n = 2048
    g = torch.Generator().manual_seed(rank)
    anchor = torch.zeros(n, device=di.device)
    w = (1e-3 * torch.randn(n, generator=g)).to(di.device)
    rows = c.all_gather(s.mask_(w, anchor, rank, 0, range(world)))
    torch.cuda.synchronize()
    torch.save({"public": dict(s.public), "pair": s.pair_words(rank, 1 - rank).tolist(), "w": w.cpu(),
                "check": sa.check_block_sum([rows[r] for r in range(world)]).cpu()}, os.path.join(outdir, f"k{rank}.pt"))
    c.close()
    comm.shutdown()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs (RCCL, one rank per GPU)")
def test_setup_keys_over_rccl_two_gpus(tmp_path):
    """Two ranks, one GPU each, ``--comm rccl``'s communicator: both learn both public keys, derive the same
    pair key, and their masked payloads' check blocks sum to 2."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_two_gpu_keys_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    st = [torch.load(tmp_path / f"k{r}.pt", weights_only=False) for r in range(2)]
    assert st[0]["public"] == st[1]["public"] and len(set(st[0]["public"].values())) == 2
    assert st[0]["pair"] == st[1]["pair"]
    assert st[0]["check"].tolist() == st[1]["check"].tolist() == [2] * 16


def _batch(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(S // 3, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids = ids * mask
    ids[:, 0] = 101
    labels = torch.randint(0, 2, (B,), generator=g)
    return ids.cuda(), mask.cuda(), labels.cuda(), int(lens.sum())


def test_secure_aggregator_on_a_model_arena():
    """``SecureAggregator`` on the default DistilBERT arena: three clients mask over two rounds, no payload
    shows its plaintext, the unmasked mean is within the fixed-point bound of the true mean (per element
    3 clients x 2^-(f+1), times 1 / 3, plus the two roundings of the chain), the pads stay +0, the shadow
    the kernel wrote is the shadow a refresh would write, and a graphed training step runs on the
    result."""
    model = DDoSClassifier(device=DEV, impl="hip", seed=3)
    A = model.arena
    n = A.numel
    assert n % 16 == 0
    live = torch.zeros(n, dtype=torch.bool, device=DEV)
    for name in A.names():
        off, shape = A.offsets[name]
        live[off:off + math.prod(shape)] = True
    agg = sa.SecureAggregator(F, 20, seed=77)
    agg.setup_keys(range(3), 3)
    g = torch.Generator(device=DEV).manual_seed(5)
    _, k0 = _keys(0)
    for r in range(2):
        anchor = A.master.clone()
        trained = [anchor + 1e-4 * (k + 1) * torch.randn(n, device=DEV, generator=g) * live for k in range(3)]
        ps = []
        for k in range(3):
            ps.append(agg.mask_(trained[k], anchor, k, r, [0, 1, 2]))
            rep = agg.last
            v = float((trained[k] - anchor).double().norm())
            assert rep["payload_bytes"] == 4 * (n + 16) and rep["masked_with"] == 2
            assert rep["clamped"] == 0 and rep["bad_elems"] == 0 and abs(rep["update_l2"] - v) <= 2.0 ** -22 * v
            assert 0 < rep["error_l2"] <= 2.0 ** -(F + 1) * math.sqrt(n)
            q = _mask(trained[k], anchor, k0)[0]
            assert int((ps[k][:n] == q[:n]).sum()) <= 64                 # (expected: n 2^-32 of the live words)
        agg.unmask_mean_(model, ps, anchor, round=r)
        torch.cuda.synchronize()
        mean = anchor.double() + ((trained[0] - anchor).double() + (trained[1] - anchor).double()
                                  + (trained[2] - anchor).double()) / 3.0
        bound = 2.0 ** -(F + 1) + 2.0 ** -24 * (2 * float(A.master.abs().max()) + 1e-3)
        assert float((A.master.double() - mean).abs().max()) <= bound
        assert not A.master[~live].view(torch.int32).any() and not A.shadow[~live].view(torch.int16).any()
        assert torch.equal(A.shadow.view(torch.int16), A.master.to(torch.bfloat16).view(torch.int16))
    # a client that masked for another live set: the check block says so and the master stays
    before = A.master.clone()
    anchor = A.master.clone()
    same = anchor.clone()
    ps = [agg.mask_(same, anchor, 0, 2, [0, 1, 2]), agg.mask_(same, anchor, 1, 2, [0, 1]),
          agg.mask_(same, anchor, 2, 2, [0, 1, 2])]
    with pytest.raises(RuntimeError, match="round 3"):
        agg.unmask_mean_(model, ps, anchor, round=2)
    assert torch.equal(_i32(A.master), _i32(before))
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


def test_refusals():
    """The binding rejects each invalid call before any launch: the buffers keep their contents."""
    n = 2048
    mk = lambda k=n, dt=torch.float32: torch.ones(k, dtype=dt, device=DEV)  # noqa: E731
    words, grid = K.secagg_words(n), K.secagg_grid(n)
    w, a, out, sh = mk(), mk(), mk(), mk(dt=torch.bfloat16)
    p, so = mk(words, torch.int32), mk(n, torch.int32)
    keys, key = mk(16, torch.int32).view(2, 8), mk(8, torch.int32)
    part, st = mk(4 * grid, torch.float64), mk(4, torch.float64)
    ext = K.ext()
    ok_mask = dict(w=w, anchor=a, keys=keys, signs=1, payload=p, partial=part, stats=st, frac_bits=24, rounds=20,
                   round=3, first_block=0)
    ok_un = dict(payloads=[p, p.clone()], anchor=a, out=out, shadow=sh, frac_bits=24)
    ok_st = dict(out=so, key=key, nonce=[1, 2, 3], rounds=20, first_block=0)

    def bad(fn, ok, **kw):
        with pytest.raises((RuntimeError, TypeError)):
            getattr(ext, fn)(**dict(ok, **kw))

    big = mk(2 * n + 64)
    bad("secagg_mask", ok_mask, w=mk(n - 8), anchor=mk(n - 8), payload=mk(n + 8, torch.int32))   # length: n % 16
    bad("secagg_mask", ok_mask, w=mk(0), anchor=mk(0), payload=mk(16, torch.int32))
    bad("secagg_mask", ok_mask, anchor=mk(n - 16))
    bad("secagg_mask", ok_mask, w=mk(dt=torch.float64))                                          # dtype
    bad("secagg_mask", ok_mask, anchor=mk(dt=torch.bfloat16))
    bad("secagg_mask", ok_mask, keys=keys.float())
    bad("secagg_mask", ok_mask, keys=keys.long())
    bad("secagg_mask", ok_mask, payload=mk(words, torch.float32))
    bad("secagg_mask", ok_mask, payload=mk(words, torch.int64))
    bad("secagg_mask", ok_mask, partial=mk(4 * grid, torch.float32))
    bad("secagg_mask", ok_mask, stats=mk(4, torch.float32))
    bad("secagg_mask", ok_mask, w=mk(2 * n)[::2])                                                # not contiguous
    bad("secagg_mask", ok_mask, keys=mk(32, torch.int32).view(8, 4).t()[:2])
    bad("secagg_mask", ok_mask, anchor=a.cpu())                                                  # device
    bad("secagg_mask", ok_mask, keys=keys.cpu())
    bad("secagg_mask", ok_mask, payload=p.cpu())
    bad("secagg_mask", ok_mask, stats=st.cpu())
    bad("secagg_mask", ok_mask, anchor=w)                                                        # overlap
    bad("secagg_mask", ok_mask, w=big[:n], anchor=big[n // 2:n // 2 + n])
    bad("secagg_mask", ok_mask, w=big[:n], payload=big[n // 2:n // 2 + words].view(torch.int32))
    bad("secagg_mask", ok_mask, w=big[:n], keys=big[16:32].view(torch.int32).view(2, 8))
    bad("secagg_mask", ok_mask, w=big[1:n + 1])                                                  # alignment
    bad("secagg_mask", ok_mask, payload=mk(words + 4, torch.int32)[1:words + 1])
    bad("secagg_mask", ok_mask, payload=mk(words - 1, torch.int32))                              # payload extent
    bad("secagg_mask", ok_mask, payload=mk(n, torch.int32))
    bad("secagg_mask", ok_mask, payload=mk(words + 16, torch.int32))
    bad("secagg_mask", ok_mask, partial=mk(4 * grid - 1, torch.float64))
    bad("secagg_mask", ok_mask, stats=mk(3, torch.float64))
    bad("secagg_mask", ok_mask, keys=mk(16, torch.int32))                                        # keys: [P, 8]
    bad("secagg_mask", ok_mask, keys=mk(16, torch.int32).view(4, 4))
    bad("secagg_mask", ok_mask, keys=mk(128, torch.int32).view(16, 8), signs=0)                  # P <= 15
    for signs in (4, -1, 1 << 15, 1 << 40):                                                      # one bit per partner
        bad("secagg_mask", ok_mask, signs=signs)
    for f in (7, 31, 0, -24, 32):
        bad("secagg_mask", ok_mask, frac_bits=f)
        bad("secagg_unmask_mean", ok_un, frac_bits=f)
    for rounds in (0, 10, 16, 21, -8):
        bad("secagg_mask", ok_mask, rounds=rounds)
        bad("secagg_stream", ok_st, rounds=rounds)
    for kw in (dict(round=-1), dict(round=1 << 32), dict(first_block=-1), dict(first_block=(1 << 32) - n // 16),
               dict(first_block=1 << 62)):
        bad("secagg_mask", ok_mask, **kw)
    for kw in (dict(first_block=-1), dict(first_block=(1 << 32) - n // 16 + 1), dict(nonce=[1, 2]), dict(nonce=[1, 2, 3, 4]),
               dict(nonce=[-1, 0, 0]), dict(nonce=[0, 1 << 32, 0]), dict(key=mk(7, torch.int32)), dict(key=key.float()),
               dict(key=key.cpu()), dict(out=mk(n - 8, torch.int32)), dict(out=mk(0, torch.int32)), dict(out=mk()),
               dict(out=mk(2 * n, torch.int32)[::2]), dict(out=mk(n + 4, torch.int32)[1:n + 1])):
        bad("secagg_stream", ok_st, **kw)
    bad("secagg_unmask_mean", ok_un, payloads=[])                                                # M
    bad("secagg_unmask_mean", ok_un, payloads=[p] * 17)
    bad("secagg_unmask_mean", ok_un, payloads=[p, mk(words - 1, torch.int32)])                   # payload extent
    bad("secagg_unmask_mean", ok_un, payloads=[mk(n, torch.int32)])
    bad("secagg_unmask_mean", ok_un, payloads=[p.float()])                                       # dtype
    bad("secagg_unmask_mean", ok_un, out=mk(dt=torch.float64))
    bad("secagg_unmask_mean", ok_un, shadow=mk())
    bad("secagg_unmask_mean", ok_un, anchor=mk(n - 16))                                          # length
    bad("secagg_unmask_mean", ok_un, shadow=mk(n - 16, torch.bfloat16))
    bad("secagg_unmask_mean", ok_un, out=mk(n - 8), anchor=mk(n - 8), shadow=None)
    bad("secagg_unmask_mean", ok_un, payloads=[p.cpu()])                                         # device
    bad("secagg_unmask_mean", ok_un, anchor=a.cpu())
    bad("secagg_unmask_mean", ok_un, out=a)                                                      # overlap
    bad("secagg_unmask_mean", ok_un, out=big[:n], anchor=big[n // 2:n // 2 + n])
    bad("secagg_unmask_mean", ok_un, out=big[:n], payloads=[big[n // 2:n // 2 + words].view(torch.int32)])
    bad("secagg_unmask_mean", ok_un, out=big[:n], shadow=big[n // 2:n].view(torch.bfloat16))
    bad("secagg_unmask_mean", ok_un, anchor=big[:n], shadow=big[n // 2:n].view(torch.bfloat16))
    bad("secagg_unmask_mean", ok_un, out=big[1:n + 1])                                           # alignment
    for args in (100, 0, -16):
        with pytest.raises(RuntimeError):
            K.secagg_words(args)
    torch.cuda.synchronize()
    assert all(torch.equal(t, torch.ones_like(t)) for t in (w, a, out, sh, p, so, keys, key, part, st, big))
    z = torch.zeros(n, device=DEV)
    K.secagg_mask(big[:n], big[n:2 * n], torch.empty((0, 8), dtype=torch.int32, device=DEV), 0, p, part, st)   # beside w
    K.secagg_unmask_mean([p], z, out, sh)
    torch.cuda.synchronize()
    assert st.tolist() == [0.0, 0.0, 0.0, 0.0] and not p[:n].any() and bool((p[n:] == 1).all())
    assert torch.equal(big, torch.ones_like(big)) and not out.any()
