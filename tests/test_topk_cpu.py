"""The top-k sparsified update exchange on the CPU (parallel/compress.py: ``torch_topk_encode_``,
``torch_topk_decode_mean_``, ``TopKCompressor``): the torch specification against a hand-written loop,
``sent + e' == v`` bit for bit and the telescoping sum of error feedback, the tie rule and the selection
edges, the payload word by word, the decoder's guards, the configuration plumbing and its refusals, the
untouched ``none`` / ``int8`` / ``int4`` paths, the virtual run against the 2-rank gloo run bit for bit, a
dropped client's residual, and the composition with a server optimizer and with client-level privacy.

No input relies on denormals."""
import argparse
import math
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"

from importlib import import_module  # noqa: E402

config = import_module(f"{PKG}.config")
data_pkg = import_module(f"{PKG}.data")
models = import_module(f"{PKG}.models")
runner = import_module(f"{PKG}.fed.runner")
fedavg = import_module(f"{PKG}.parallel.fedavg")
cp = import_module(f"{PKG}.parallel.compress")

SEED = 0x5EEDF00DCAFE
TOPK_KEYS = ("compress_ratio", "payload_bytes", "update_l2", "quant_error_l2", "bad_elems", "sent", "threshold")
QUANT_KEYS = ("compress_ratio", "payload_bytes", "update_l2", "quant_error_l2", "bad_groups")
CH = 4096
LENGTHS = (64, CH + 64, 2 * CH + 3 * 64)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _clear_rank_env():
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)


def _single_thread(fn):
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)  # (CPU GEMM reductions split by thread count: same count on both sides)
    try:
        return fn()
    finally:
        torch.set_num_threads(nthreads)


def _bits(t):
    return t.contiguous().view(torch.int32).tolist()


def _f32(bits):
    return float(torch.tensor(bits, dtype=torch.int32).view(torch.float32))


def _vectors(n, seed, scale=0.01):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=g)
    w = a + scale * torch.randn(n, generator=g) * torch.rand(n, generator=g)
    e = 0.1 * scale * torch.randn(n, generator=g)
    return w, a, e


def _chunks(n):
    return (n + CH - 1) // CH


# ------------------------------------------------------------------ 1. the specification against a loop
def _loop_encode(w, a, e, k):
    """The module docstring, element by element, in numpy float32 scalars.  Returns (payload words as
    Python ints, new residual, stats)."""
    f = np.float32
    n = len(w)
    v, key, bad = [], [], []
    with np.errstate(all="ignore"):
        for i in range(n):
            x = f(w[i]) - f(a[i])
            if e is not None:
                x = f(x + f(e[i]))
            v.append(f(x))
            kb = int(np.array(x, dtype=np.float32).view(np.uint32)) & 0x7FFFFFFF
            key.append(kb)
            bad.append(kb >= 0x7F800000)
    cand = [i for i in range(n) if not bad[i]]
    k_eff = min(k, len(cand))
    order = sorted(cand, key=lambda i: (-key[i], i))             # largest key first, ties by the lower index
    sent = sorted(order[:k_eff])
    C = _chunks(n)
    off = [0] * (C + 1)
    for i in sent:
        off[i // CH + 1] += 1
    for b in range(C):
        off[b + 1] += off[b]
    vals = [int(np.array(v[i], dtype=np.float32).view(np.int32)) for i in sent] + [0] * (k - k_eff)
    halves = [i % CH for i in sent] + [0] * (2 * ((k + 1) // 2) - k_eff)
    idx = []
    for j in range(0, len(halves), 2):
        word = halves[j] | (halves[j + 1] << 16)
        idx.append(word - (1 << 32) if word >= 1 << 31 else word)
    s = set(sent)
    res = [f(0) if (i in s or bad[i]) else v[i] for i in range(n)]
    sv = sum(float(v[i]) ** 2 for i in range(n) if not bad[i])
    se = sum(float(res[i]) ** 2 for i in range(n) if not bad[i])
    thr = min(abs(float(v[i])) for i in sent) if sent else 0.0
    stats = {"update_l2": float(f(math.sqrt(sv))), "error_l2": float(f(math.sqrt(se))), "bad_elems": sum(bad),
             "sent": k_eff, "threshold": thr}
    return off + vals + idx, res, stats


def _check_against_loop(w, a, e, k):
    want_p, want_e, want_s = _loop_encode(w.tolist(), a.tolist(), None if e is None else e.tolist(), k)
    got_e = None if e is None else e.clone()
    payload, stats = cp.torch_topk_encode_(w, a, got_e, k)
    assert payload.dtype == torch.int32 and payload.numel() == cp.topk_words(w.numel(), k) == len(want_p)
    assert payload.tolist() == want_p
    if e is not None:
        assert _bits(got_e) == _bits(torch.tensor(np.array(want_e, dtype=np.float32)))
    for key in ("bad_elems", "sent", "threshold"):
        assert stats[key] == want_s[key], key
    for key in ("update_l2", "error_l2"):  # (fp64 sums in another order: the fp32 roots one ulp apart at most)
        assert abs(stats[key] - want_s[key]) <= 2.0 ** -23 * want_s[key], key
    return payload, got_e, stats


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("feedback", [True, False])
def test_specification_equals_the_loop(n, feedback):
    w, a, e = _vectors(n, seed=n)
    for k in sorted({1, max(1, n // 100), 7 if n > 64 else 3, n // 2}):
        _check_against_loop(w, a, e if feedback else None, k)
    assert cp.topk_k(n, 0.01) == max(1, n // 100) and cp.topk_k(n, 0.5) == n // 2 and cp.topk_k(64, 1e-9) == 1
    assert cp.topk_words(n, 5) == _chunks(n) + 1 + 5 + 3


# ------------------------------------------------------------------ 2. nothing is lost
@pytest.mark.parametrize("n", LENGTHS)
def test_sent_plus_residual_is_the_update_bitwise(n):
    w, a, e = _vectors(n, seed=3 * n + 1)
    k = max(1, n // 10)
    v = (w - a) + e
    res = e.clone()
    payload, stats = cp.torch_topk_encode_(w, a, res, k)
    zero, dense = torch.zeros(n), torch.empty(n)
    cp.torch_topk_decode_mean_([payload], zero, dense, None, k)          # 0 + val * 1: exact
    assert _bits(dense + res) == _bits(v)
    assert int((dense != 0).sum()) == k == stats["sent"] and not bool(((dense != 0) & (res != 0)).any())
    assert float(dense[dense != 0].abs().min()) == stats["threshold"] >= float(res.abs().max())


def test_error_feedback_telescopes():
    """Over 4 rounds sum(sent) = sum(updates) - e_T.  ``sent + e' == v`` is exact, so per round and
    element one rounding (v = update + e, within 2^-24 |v|) separates the two sides."""
    n, T, k = CH + 64, 4, 40
    zero = torch.zeros(n)
    e = torch.zeros(n)
    sent, total = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    vmax = 0.0
    for r in range(T):
        upd = _vectors(n, seed=100 + r)[2]
        vmax = max(vmax, float((upd + e).abs().max()))
        payload, stats = cp.torch_topk_encode_(upd, zero, e, k)
        out = torch.empty(n)
        cp.torch_topk_decode_mean_([payload], zero, out, None, k)
        sent += out.double()
        total += upd.double()
        assert abs(stats["error_l2"] - float(e.double().norm())) <= 2.0 ** -23 * stats["error_l2"]
    gap = (sent - (total - e.double())).abs().max()
    assert float(gap) <= T * 2.0 ** -24 * vmax
    assert float(e.abs().max()) > 0
    sent2 = torch.zeros(n, dtype=torch.float64)                           # without feedback the rest is dropped
    for r in range(T):
        payload, _ = cp.torch_topk_encode_(_vectors(n, seed=100 + r)[2], zero, None, k)
        out = torch.empty(n)
        cp.torch_topk_decode_mean_([payload], zero, out, None, k)
        sent2 += out.double()
    assert float((sent2 - total).abs().max()) > 100 * float(gap + 1e-12)


# ------------------------------------------------------------------ 3. ties and the selection edges
def _sent_indices(payload, n, k):
    off, val, loc = cp.split_topk_payload(payload, n, k)
    sent = int(off[-1])
    chunk = torch.repeat_interleave(torch.arange(_chunks(n)), (off[1:] - off[:-1]).to(torch.int64))
    return (chunk * CH + loc[:sent]).tolist(), val[:sent]


def test_ties_and_selection_edges():
    n = 2 * CH + 3 * 64
    zero = torch.zeros(n)
    # all values equal: the k lowest indices
    w = torch.full((n,), 0.5)
    p, e, st = _check_against_loop(w, zero, zero.clone(), 100)
    assert _sent_indices(p, n, 100)[0] == list(range(100)) and st["threshold"] == 0.5
    assert not e[:100].any() and bool((e[100:] == 0.5).all())
    # a tie group that straddles the chunk boundary and is cut by the budget: 3 above, 6 tied, k = 7
    w = 1e-3 * _vectors(n, seed=5)[2]
    ties = [CH - 3, CH - 1, CH, CH + 2, 2 * CH - 1, 2 * CH + 5]
    w[ties] = torch.tensor([0.25, -0.25, 0.25, -0.25, 0.25, 0.25])
    w[[7, CH + 9, 2 * CH + 100]] = torch.tensor([1.0, -2.0, 3.0])
    p, e, st = _check_against_loop(w, zero, zero.clone(), 7)
    idx, val = _sent_indices(p, n, 7)
    assert idx == sorted([7, CH + 9, 2 * CH + 100] + ties[:4]) and st["threshold"] == 0.25
    assert e[ties[4]] == 0.25 and e[ties[5]] == 0.25 and not e[ties[:4]].any()
    assert cp.split_topk_payload(p, n, 7)[0].tolist() == [0, 3, 6, 7]
    # all zeros: zeros are sent, lowest index first; the payload keeps its size
    p, e, st = _check_against_loop(zero, zero, zero.clone(), 5)
    assert _sent_indices(p, n, 5)[0] == [0, 1, 2, 3, 4] and st["sent"] == 5 and st["threshold"] == 0.0
    assert not p[_chunks(n) + 1:_chunks(n) + 6].any() and st["update_l2"] == 0.0      # (the values: +0)
    # -0 has key 0: it ties with +0 and, sent, keeps its sign bit
    w = zero.clone()
    w[3] = -0.0
    w[10] = 1.0
    p, _, st = _check_against_loop(w, zero, None, 5)                   # (with a residual: -0 + +0 = +0)
    idx, val = _sent_indices(p, n, 5)
    assert idx == [0, 1, 2, 3, 10] and _bits(val) == [0, 0, 0, -(1 << 31), _bits(torch.tensor([1.0]))[0]]
    # fewer nonzero candidates than k: the nonzero ones, then zeros from index 0
    w = zero.clone()
    w[[50, CH + 1]] = torch.tensor([-2.0, 1.0])
    p, _, st = _check_against_loop(w, zero, None, 4)
    assert _sent_indices(p, n, 4)[0] == [0, 1, 50, CH + 1] and st["threshold"] == 0.0
    # k = 1 and k = n / 2
    w, a, e0 = _vectors(n, seed=8)
    p, _, st = _check_against_loop(w, a, e0, 1)
    v = (w - a) + e0
    assert _sent_indices(p, n, 1)[0] == [int(v.abs().argmax())] and st["threshold"] == float(v.abs().max())
    p, e, st = _check_against_loop(w, a, e0, n // 2)
    assert st["sent"] == n // 2 and int((e == 0).sum()) >= n // 2


def test_bad_elements():
    n = 64
    zero = torch.zeros(n)
    w = 0.01 * torch.arange(1, n + 1, dtype=torch.float32)
    w[[5, 9]] = torch.tensor([float("nan"), float("-inf")])
    p, e, st = _check_against_loop(w, zero, zero.clone(), 3)
    assert st["bad_elems"] == 2 and st["sent"] == 3 and _sent_indices(p, n, 3)[0] == [61, 62, 63]
    assert _bits(e[[5, 9]]) == [0, 0] and bool(torch.isfinite(e).all()) and math.isfinite(st["update_l2"])
    # n - bad < k: 60 NaNs, k = 8 -> the four candidates are sent, entries 4 .. 8 are 0
    w = torch.full((n,), float("nan"))
    w[[3, 17, 40, 63]] = torch.tensor([1.0, 0.0, -3.0, 2.0])
    p, e, st = _check_against_loop(w, zero, zero.clone(), 8)
    assert st["bad_elems"] == 60 and st["sent"] == 4 and st["threshold"] == 0.0
    off, val, loc = cp.split_topk_payload(p, n, 8)
    assert off.tolist() == [0, 4] and loc.tolist() == [3, 17, 40, 63, 0, 0, 0, 0]
    assert val.tolist() == [1.0, 0.0, -3.0, 2.0, 0.0, 0.0, 0.0, 0.0] and not e.view(torch.int32).any()
    # every element bad: nothing is sent, the threshold is 0
    p, e, st = _check_against_loop(torch.full((n,), float("inf")), zero, zero.clone(), 2)
    assert st["bad_elems"] == 64 and st["sent"] == 0 and st["threshold"] == 0.0 and not p.any() and not e.any()
    # 3e38 - (-3e38) overflows: bad
    w, a = torch.full((n,), 0.5), torch.zeros(n)
    w[7], a[7] = 3e38, -3e38
    p, e, st = _check_against_loop(w, a, None, 2)
    assert st["bad_elems"] == 1 and _sent_indices(p, n, 2)[0] == [0, 1]


# ------------------------------------------------------------------ 4. the payload, word by word
def test_payload_layout_and_pads():
    n, k = 2 * CH + 3 * 64, 5
    zero = torch.zeros(n)
    w = zero.clone()
    where = [70, CH - 1, CH, 2 * CH + 64, 2 * CH + 127]
    w[where] = torch.tensor([1.5, -2.5, 3.5, -4.5, 5.5])
    w[100] = 0.125                                                     # the largest entry not sent
    e = zero.clone()
    p, st = cp.torch_topk_encode_(w, zero, e, k)
    C = 3
    assert p.numel() == cp.topk_words(n, k) == C + 1 + 5 + 3
    assert p[:C + 1].tolist() == [0, 2, 3, 5]
    assert p[C + 1:C + 6].tolist() == _bits(torch.tensor([1.5, -2.5, 3.5, -4.5, 5.5]))
    assert p[C + 6:].tolist() == [70 | (4095 << 16), 0 | (64 << 16), 127]        # the unused half is 0
    assert st == {"update_l2": st["update_l2"], "error_l2": 0.125, "bad_elems": 0, "sent": 5, "threshold": 1.5}
    assert float(e[100]) == 0.125 and int((e != 0).sum()) == 1
    assert cp.split_topk_payload(p, n, k)[2].tolist() == [70, 4095, 0, 64, 127]
    # 64-float pads (+0 in w, anchor and e) stay +0 through both, sent (as zeros) or not
    w3, a3, e3 = _vectors(n, seed=4)
    for lo in (0, n - 64):
        w3[lo:lo + 64] = 0.0
        a3[lo:lo + 64] = 0.0
        e3[lo:lo + 64] = 0.0
    for k3 in (20, n // 2):
        r3 = e3.clone()
        p3, _ = cp.torch_topk_encode_(w3, a3, r3, k3)
        out = torch.empty(n)
        sh = torch.empty(n, dtype=torch.bfloat16)
        cp.torch_topk_decode_mean_([p3, p3], a3, out, sh, k3)
        for lo in (0, n - 64):
            assert not r3[lo:lo + 64].view(torch.int32).any() and not out[lo:lo + 64].view(torch.int32).any()
        assert torch.equal(sh.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))


# ------------------------------------------------------------------ 5. decode: the sum's order and the guards
def _loop_decode(payloads, anchor, n, k):
    f = np.float32
    C = _chunks(n)
    acc = [f(0)] * n
    for p in payloads:
        p = p.tolist()
        off, vals, words = p[:C + 1], p[C + 1:C + 1 + k], p[C + 1 + k:]
        for b in range(C):
            lo = min(max(off[b], 0), k)
            hi = min(max(off[b + 1], lo), k)
            length = min(CH, n - b * CH)
            for j in range(lo, hi):
                word = words[j // 2] & 0xFFFFFFFF
                li = (word >> 16) if j & 1 else (word & 0xFFFF)
                if li < length:
                    acc[b * CH + li] = f(acc[b * CH + li] + f(_f32(vals[j])))
    inv = f(1.0 / len(payloads))
    return [f(f(anchor[i]) + f(acc[i] * inv)) for i in range(n)]


def test_decode_mean_order_and_guards():
    n, k = CH + 64, 6
    a = _vectors(n, seed=2)[1]
    zero = torch.zeros(n)
    ps = []
    for c in range(3):
        w = a.clone()
        w[[5, 200 + c, CH + 10]] += torch.tensor([0.5 * (c + 1), -1.0, 2.0 ** -c])
        ps.append(cp.torch_topk_encode_(w, a, None, k)[0])
    for M in (1, 2, 3):
        out = torch.empty(n)
        cp.torch_topk_decode_mean_(ps[:M], a, out, None, k)
        assert _bits(out) == _bits(torch.tensor(np.array(_loop_decode(ps[:M], a.tolist(), n, k), dtype=np.float32)))
    # the order of the payloads is the order of the fp32 sum: (1e8 - 1e8) + 1 = 1, (1e8 + 1) - 1e8 = 0
    one = []
    for x in (1e8, -1e8, 1.0):
        w = zero.clone()
        w[77] = x
        one.append(cp.torch_topk_encode_(w, zero, None, 1)[0])
    out = torch.empty(n)
    cp.torch_topk_decode_mean_(one, zero, out, None, 1)
    assert float(out[77]) == float(np.float32(1.0) * np.float32(1.0 / 3))
    cp.torch_topk_decode_mean_([one[0], one[2], one[1]], zero, out, None, 1)
    assert float(out[77]) == 0.0
    # guards: a descending offset, an offset above k, a negative one, a local index beyond the ragged chunk
    C = 2
    good = ps[0]
    for name, edit in (("descending", lambda p: p.__setitem__(1, 1) or p.__setitem__(2, 0)),
                       ("above k", lambda p: p.__setitem__(2, k + 8)),
                       ("first above k", lambda p: p.__setitem__(0, k + 3)),
                       ("negative", lambda p: p.__setitem__(1, -4)),
                       ("beyond the ragged chunk", lambda p: p.__setitem__(C + 1 + k + 2, 64 | (4095 << 16)))):
        bad = good.clone()
        bad[C + 1 + k + 2] = 10 | (63 << 16)                     # entries 4 and 5 of the ragged chunk
        edit(bad)
        out = torch.empty(n)
        cp.torch_topk_decode_mean_([bad, ps[1]], a, out, None, k)
        want = _loop_decode([bad, ps[1]], a.tolist(), n, k)
        assert _bits(out) == _bits(torch.tensor(np.array(want, dtype=np.float32))), name
        assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ 6. plumbing and refusals
def _cfg(outdir, rounds, **kw):
    base = dict(out_dir=outdir, synthetic_rows=600, data_fraction=0.1, max_len=32, epochs=1, batch_size=8,
                eval_batch_size=16, plots=False, resume=False, rounds=rounds, verbose=False, heartbeat_s=0.0,
                save_checkpoints=False)
    base.update(kw)
    return config.FedConfig(**base)


def _client(cfg, frame):
    return runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1)).setup()


def test_config_env_and_cli_reach_the_runner(monkeypatch, tmp_path):
    d = config.FedConfig()
    assert (d.compress, d.compress_density) == ("none", 0.01)
    parser = config.FedConfig.add_cli(argparse.ArgumentParser())
    cfg = config.FedConfig.from_args(parser.parse_args(
        ["--compress", "topk", "--compress-density", "0.001", "--compress-error-feedback", "false"]))
    assert (cfg.compress, cfg.compress_density, cfg.compress_error_feedback) == ("topk", 0.001, False)
    monkeypatch.setenv("FEDDDOS_COMPRESS", "topk")
    monkeypatch.setenv("FEDDDOS_COMPRESS_DENSITY", "0.05")
    cfg = config.FedConfig.from_args(parser.parse_args([]))
    assert (cfg.compress, cfg.compress_density, cfg.compress_error_feedback) == ("topk", 0.05, True)
    cfg = config.FedConfig.from_args(parser.parse_args(["--compress-density", "0.25"]))  # flags win
    assert cfg.compress == "topk" and cfg.compress_density == 0.25
    _clear_rank_env()
    for k, v in dict(out_dir=str(tmp_path), synthetic_rows=600, max_len=32, plots=False, resume=False, verbose=False,
                     heartbeat_s=0.0).items():
        setattr(cfg, k, v)
    c = _client(cfg, None).compress
    assert isinstance(c, cp.TopKCompressor) and (c.density, c.error_feedback) == (0.25, True)
    assert c.describe() == "top-k, density 0.25" and c.k(6400) == 1600 and c.words(6400) == 2 + 1 + 1600 + 800
    monkeypatch.delenv("FEDDDOS_COMPRESS")
    # a density without compress=topk is ignored, whatever its value
    assert _client(_cfg(str(tmp_path), 1), None).compress is None
    monkeypatch.delenv("FEDDDOS_COMPRESS_DENSITY")
    assert cp.make_compressor(_cfg(str(tmp_path), 1, compress_density=7.0)) is None
    q = cp.make_compressor(_cfg(str(tmp_path), 1, compress="int8", compress_density=-1.0))
    assert type(q) is cp.Compressor and q.describe() == "int8" and q.words(128) == cp.payload_words(128, 8)
    assert cp.check_compress_config(_cfg(str(tmp_path), 1, compress="topk")) == -1
    off = cp.make_compressor(_cfg(str(tmp_path), 1, compress="topk", compress_error_feedback=False))
    assert not off.error_feedback and off.residual(0, torch.zeros(64)) is None
    # refused at setup, before any work, with a message naming the flag
    for kw, match in ((dict(compress_density=0.0), "compress_density"), (dict(compress_density=-0.1), "compress_density"),
                      (dict(compress_density=0.500001), "compress_density"),
                      (dict(compress_density=float("nan")), "compress_density"),
                      (dict(compress_rounding="stochastic"), "compress_rounding"),
                      (dict(compress_rounding="up"), "compress_rounding"),
                      (dict(transport="tcp"), "transport"), (dict(aggregator="median"), "aggregator"),
                      (dict(aggregator="trimmed_mean"), "aggregator"), (dict(weighted_fedavg=True), "weighted_fedavg")):
        with pytest.raises(ValueError, match=match):
            _client(_cfg(str(tmp_path), 1, compress="topk", **kw), None)
    with pytest.raises(ValueError, match="gpus_per_client"):
        cp.make_compressor(_cfg(str(tmp_path), 1, compress="topk"), gpus_per_client=2)
    with pytest.raises(ValueError, match="compress"):
        _client(_cfg(str(tmp_path), 1, compress="top-k"), None)
    for density in (0.0, 0.6, -1.0):
        with pytest.raises(ValueError):
            cp.TopKCompressor(density)
    w, a, _ = _vectors(128, seed=1)
    for args in ((w, a[:64], None, 4), (w, a.double(), None, 4), (w[:100], a[:100], None, 4), (w, a, None, 0),
                 (w, a, None, 65), (w, a, w[:64], 4)):
        with pytest.raises(ValueError):
            cp.torch_topk_encode_(*args)
    p = cp.torch_topk_encode_(w, a, None, 4)[0]
    out = torch.empty(128)
    for plist, k in (([], 4), ([p] * 17, 4), ([p], 5), ([p[:-1]], 4), ([p.float()], 4)):
        with pytest.raises(ValueError):
            cp.torch_topk_decode_mean_(plist, a, out, None, k)
    model = types.SimpleNamespace(arena=types.SimpleNamespace(master=w))
    with pytest.raises(ValueError, match="anchor"):
        fedavg.fedavg_(model, compress=cp.TopKCompressor(0.1))
    with pytest.raises(ValueError, match="robust"):
        fedavg.fedavg_(model, compress=cp.TopKCompressor(0.1), anchor=a, robust=object())


# ------------------------------------------------------------------ 7. none / int8 / int4 untouched
def test_the_other_modes_are_untouched(tmp_path, monkeypatch):
    """``compress="none"`` never reaches a compressor; int8 / int4 keep their record keys and their log
    lines, character for character."""
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)

    def boom(*a, **k):
        raise AssertionError("reached the sparsifier")

    monkeypatch.setattr(cp.TopKCompressor, "encode_", boom)
    monkeypatch.setattr(cp.TopKCompressor, "decode_mean_", boom)
    monkeypatch.setattr(cp, "torch_topk_encode_", boom)
    monkeypatch.setattr(cp, "torch_topk_decode_mean_", boom)
    solo = _client(_cfg(str(tmp_path / "solo"), 1), frame)
    rec = _single_thread(lambda: solo.run_round(0))
    assert solo.compress is None and not any(k in rec for k in set(TOPK_KEYS) | set(QUANT_KEYS))
    for mode, ratio in (("int8", "3.76"), ("int4", "7.11")):
        lines, said = [], []
        client = runner.FederatedClient(_cfg(str(tmp_path / mode), 1, compress=mode), frame=frame,
                                        model_config=models.DistilBertConfig(n_layers=1))
        client.log.info = lambda msg, *a, **k: lines.append(msg)
        client.setup()
        assert (f"quantized update exchange: {mode}, nearest rounding, error feedback on (payload {ratio}x smaller than "
                f"fp32)") in lines
        res = _single_thread(lambda: runner.run_virtual_clients(client, 2, rounds=1, progress=said.append))
        h = res["rounds"][0]
        n = client.model.arena.master.numel()
        nbytes = 4 * cp.payload_words(n, int(mode[3:]))
        for c in h["clients"]:
            assert all(k in c for k in QUANT_KEYS) and not any(k in c for k in ("bad_elems", "sent", "threshold"))
        assert "bad_groups" in h and not any(k in h for k in ("bad_elems", "sent"))
        er = math.sqrt(sum(c["quant_error_l2"] ** 2 for c in h["clients"]))
        up = math.sqrt(sum(c["update_l2"] ** 2 for c in h["clients"]))
        assert (f"round 1/1 quantized exchange: {mode}, {nbytes} B per client ({float(ratio):.2f}x smaller), pooled "
                f"|quantization error| = {er:.6g} of |update| = {up:.6g}") in said
        one = _client(_cfg(str(tmp_path / (mode + "one")), 1, compress=mode), frame)
        one.log.info = lambda msg, *a, **k: lines.append(msg)
        rec = _single_thread(lambda: one.run_round(0))
        assert all(k in rec for k in QUANT_KEYS) and not any(k in rec for k in ("bad_elems", "sent", "threshold"))
        assert (f"quantized update: {rec['payload_bytes']} B sent ({rec['compress_ratio']:.2f}x smaller), |update| = "
                f"{rec['update_l2']:.6g}, |quantization error| = {rec['quant_error_l2']:.6g}") in lines


# ------------------------------------------------------------------ 8. virtual == 2-rank gloo
def _fed_worker(rank, world, port, outdir, rounds, kw):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    comm = import_module(f"{PKG}.parallel.comm")
    comm.init_distributed(device="cpu")
    torch.set_num_threads(1)
    cfg = _cfg(outdir, rounds, **kw)
    frame = data_pkg.generate_cicids2017(cfg.synthetic_rows, seed=0)
    client = runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1))
    client.setup()
    for r in range(client.start_round, cfg.rounds):
        client.run_round(r)
    torch.save({"master": client.model.arena.master.clone(), "history": client.history,
                "residual": client.compress.residuals[rank].clone()}, os.path.join(outdir, f"state_rank{rank}.pt"))
    client.log.close()
    comm.shutdown()


def test_virtual_equals_two_rank_gloo_run(tmp_path):
    """tests/test_virtual_rounds.py's configuration with the sparsified exchange at density 0.01 and error
    feedback over 2 rounds (so round 2 encodes with a residual): the virtual run and the 2-rank gloo run
    agree bit for bit -- weights, residuals and records."""
    world, rounds = 2, 2
    real = tmp_path / "real"
    real.mkdir()
    kw = dict(synthetic_rows=1500, max_len=64, compress="topk", compress_density=0.01)
    mp.spawn(_fed_worker, args=(world, _free_port(), str(real), rounds, kw), nprocs=world, join=True)
    _clear_rank_env()
    cfg = _cfg(str(tmp_path / "virtual"), rounds, **kw)
    frame = data_pkg.generate_cicids2017(cfg.synthetic_rows, seed=0)

    def virtual():
        client = _client(cfg, frame)
        init = client.model.arena.master.clone()
        return client, init, runner.run_virtual_clients(client, world, rounds=rounds)

    client, init, res = _single_thread(virtual)
    st = [torch.load(real / f"state_rank{r}.pt", weights_only=False) for r in range(world)]
    assert torch.equal(st[0]["master"], st[1]["master"])
    assert torch.equal(st[0]["master"], client.model.arena.master) and not torch.equal(init, st[0]["master"])
    n = client.model.arena.master.numel()
    k = cp.topk_k(n, 0.01)
    for rank in range(world):
        assert _bits(st[rank]["residual"]) == _bits(client.compress.residuals[rank]) and bool(st[rank]["residual"].any())
    for r in range(rounds):
        got = res["rounds"][r]
        assert got["payload_bytes"] == 4 * cp.topk_words(n, k) and got["sent"] == world * k and got["bad_elems"] == 0
        for rank in range(world):
            want, c = st[rank]["history"][r], got["clients"][rank]
            for key in TOPK_KEYS:
                assert c[key] == want[key], (rank, r, key)
            assert c["bad_elems"] == 0 and c["sent"] == k and c["threshold"] > 0
            assert 0 < c["quant_error_l2"] < c["update_l2"] and c["compress_ratio"] > 60
            assert c["aggregated_test"]["loss"] == want["aggregated_test"]["loss"], (rank, r)
            assert c["local_test"]["loss"] == want["local_test"]["loss"], (rank, r)


# ------------------------------------------------------------------ 9. a dropped client
def _drop_worker(rank, world, port, outdir):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    comm = import_module(f"{PKG}.parallel.comm")
    comm.init_distributed(device="cpu")
    torch.set_num_threads(1)
    model = models.DDoSClassifier(config=models.DistilBertConfig(n_layers=1), device="cpu", impl="torch", seed=0)
    A = model.arena
    live = torch.zeros(A.numel, dtype=torch.bool)
    for off, shape in A.offsets.values():
        live[off:off + math.prod(shape)] = True
    c = cp.TopKCompressor(0.01)
    out = {}
    for r, participate in enumerate((True, rank == 0)):           # round 2: rank 1 is dropped
        anchor = A.master.clone()
        g = torch.Generator().manual_seed(10 * r + rank)
        with torch.no_grad():
            A.master.add_(1e-3 * torch.randn(A.numel, generator=g) * live)
        sent = A.master.clone()
        before = c.residuals[rank].clone() if rank in c.residuals else None
        total = fedavg.fedavg_(model, participate=participate, comm=None, compress=c, anchor=anchor, client=rank, round=r)
        out[r] = {"total": total, "anchor": anchor, "sent": sent, "before": before,
                  "after": c.residuals[rank].clone(), "master": A.master.clone(), "last": c.last}
    torch.save(out, os.path.join(outdir, f"drop_rank{rank}.pt"))
    comm.shutdown()


def test_a_dropped_client_keeps_its_residual(tmp_path):
    world = 2
    mp.spawn(_drop_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    st = [torch.load(tmp_path / f"drop_rank{r}.pt", weights_only=False) for r in range(world)]
    for r in range(2):
        assert torch.equal(st[0][r]["master"], st[1][r]["master"])          # the ranks stay identical
    assert st[0][0]["total"] == st[1][0]["total"] == 2.0 and st[0][1]["total"] == st[1][1]["total"] == 1.0
    # rank 1, dropped from round 2: nothing encoded, the residual as round 1 left it
    assert st[1][1]["last"] is None and bool(st[1][1]["before"].any())
    assert _bits(st[1][1]["after"]) == _bits(st[1][1]["before"]) == _bits(st[1][0]["after"])
    assert _bits(st[0][1]["after"]) != _bits(st[0][1]["before"])
    # the aggregate of round 2 is rank 0's scattered update alone; of round 1 the mean of both, in client order
    n = st[0][1]["sent"].numel()
    k = cp.topk_k(n, 0.01)
    res = st[0][1]["before"].clone()
    p0 = cp.torch_topk_encode_(st[0][1]["sent"], st[0][1]["anchor"], res, k)[0]
    want = torch.empty(n)
    cp.torch_topk_decode_mean_([p0], st[0][1]["anchor"], want, None, k)
    assert _bits(want) == _bits(st[0][1]["master"]) and _bits(res) == _bits(st[0][1]["after"])
    ps = [cp.torch_topk_encode_(st[r][0]["sent"], st[r][0]["anchor"], None, k)[0] for r in range(world)]
    cp.torch_topk_decode_mean_(ps, st[0][0]["anchor"], want, None, k)
    assert _bits(want) == _bits(st[0][0]["master"])
    # one process, not sampled: the same
    c = cp.TopKCompressor(0.01)
    model = types.SimpleNamespace(arena=types.SimpleNamespace(master=st[0][0]["sent"].clone(), shadow=None),
                                  sync_shadow=lambda force=False: None)
    assert fedavg.fedavg_(model, participate=False, compress=c, anchor=st[0][0]["anchor"]) == 0.0
    assert not c.residuals and c.last is None and torch.equal(model.arena.master, st[0][0]["sent"])


# ------------------------------------------------------------------ 10. composition, order, log and record
@pytest.mark.parametrize("kw,keys", [(dict(server_opt="adam", server_lr=0.01), ("delta_l2", "step_l2")),
                                     (dict(privacy_clip=0.01, privacy_noise=0.2, privacy_seed=SEED),
                                      ("privacy_epsilon",))])
def test_composes_with_the_other_features(tmp_path, kw, keys):
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    client = _client(_cfg(str(tmp_path), 2, compress="topk", compress_density=0.01, **kw), frame)
    order, said = [], []
    if client.privacy is not None:
        real_priv = client.privacy.privatize_
        client.privacy.privatize_ = lambda *a, **k: (order.append("privatize"), real_priv(*a, **k))[1]
    real_enc = client.compress.encode_
    client.compress.encode_ = lambda *a, **k: (order.append("encode"), real_enc(*a, **k))[1]
    res = _single_thread(lambda: runner.run_virtual_clients(client, 2, rounds=2, progress=said.append))
    assert bool(torch.isfinite(client.model.arena.master).all())
    if "privacy_clip" in kw:
        assert order == ["privatize", "encode"] * 4
    else:
        assert order == ["encode"] * 4 and client.server.rounds == 2
    k = client.compress.k(client.model.arena.master.numel())
    for h in res["rounds"]:
        assert all(key in h for key in keys) and h["bad_elems"] == 0 and h["sent"] == 2 * k and h["quant_error_l2"] > 0
        assert "bad_groups" not in h
        for c in h["clients"]:
            assert all(key in c for key in TOPK_KEYS) and c["quant_error_l2"] > 0
            assert c["sent"] == k and c["threshold"] > 0 and "bad_groups" not in c
            if "privacy_clip" in kw:   # privacy's update_l2 (before the clip) stays; what is held back is mostly noise
                assert c["clipped"] == 1 and c["update_l2"] > 0.01
            else:
                assert c["quant_error_l2"] < c["update_l2"]
    assert any("sparsified exchange: top-k, density 0.01" in m and "pooled |held back|" in m for m in said)
    assert len(client.compress.residuals) == 2 and all(bool(e.any()) for e in client.compress.residuals.values())


def test_run_round_order_log_and_record(tmp_path):
    """run_round in one process: privatize, then poison, then encode; the log line and the record carry
    the sparsifier's keys; an elastic restart says that the residual starts again from zero."""
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    os.environ["TORCHELASTIC_RESTART_COUNT"] = "1"
    try:
        lines = []
        cfg = _cfg(str(tmp_path), 1, compress="topk", compress_density=0.001, privacy_clip=1e-3, privacy_seed=SEED,
                   poison_client=0, poison_kind="scale", poison_scale=1.0, verbose=False)
        client = runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1))
        client.log.info = lambda msg, *a, **k: lines.append(msg)
        client.setup()
    finally:
        del os.environ["TORCHELASTIC_RESTART_COUNT"]
    assert "sparsified update exchange: top-k, density 0.001, error feedback on (about 6 bytes per sent entry)" in lines
    assert any("sparsification residual" in m and "from zero" in m for m in lines)
    order = []
    real_priv, real_enc, real_poison = client.privacy.privatize_, client.compress.encode_, runner.faults.poison_
    client.privacy.privatize_ = lambda *a, **k: (order.append("privatize"), real_priv(*a, **k))[1]
    client.compress.encode_ = lambda *a, **k: (order.append("encode"), real_enc(*a, **k))[1]
    try:
        runner.faults.poison_ = lambda *a, **k: (order.append("poison"), real_poison(*a, **k))[1]
        rec = _single_thread(lambda: client.run_round(0))
    finally:
        runner.faults.poison_ = real_poison
    assert order == ["privatize", "poison", "encode"]
    n = client.model.arena.master.numel()
    k = cp.topk_k(n, 0.001)
    assert rec["payload_bytes"] == 4 * cp.topk_words(n, k) and rec["compress_ratio"] == n / cp.topk_words(n, k) > 500
    assert rec["bad_elems"] == 0 and rec["sent"] == k and rec["threshold"] > 0 and rec["quant_error_l2"] > 0
    assert rec["clipped"] == 1 and "bad_groups" not in rec
    assert any(m.startswith(f"sparsified update: {k} entries >= ") and "|held back| = " in m for m in lines)
