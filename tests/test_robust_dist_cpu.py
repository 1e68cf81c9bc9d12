"""Multi-Krum and the geometric median on the CPU (parallel/robust_dist.py; Blanchard et al. NeurIPS 2017,
Pillutla et al. IEEE TSP 2022): the torch specification against hand-written per-element loops,
``krum_select`` against a brute-force enumeration, its tie rule and non-finite entries, the Weiszfeld
properties on the inputs the specification was tried on, the configuration plumbing and its refusals, the
untouched default path, the virtual run against the 3-rank gloo run bit for bit, a dropped client, a client
that lies, one liar too many, and the composition with a server optimizer and with client-level privacy."""
import argparse
import dataclasses
import itertools
import json
import math
import os
import socket
import struct
import types

import pytest
import torch
import torch.multiprocessing as mp

PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"

from importlib import import_module  # noqa: E402

config = import_module(f"{PKG}.config")
data_pkg = import_module(f"{PKG}.data")
models = import_module(f"{PKG}.models")
runner = import_module(f"{PKG}.fed.runner")
rb = import_module(f"{PKG}.parallel.robust")
rd = import_module(f"{PKG}.parallel.robust_dist")
so = import_module(f"{PKG}.parallel.server_opt")

NEW_FIELDS = ("byzantine", "krum_select", "geomed_iters", "geomed_nu")
NAN = float("nan")


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


class FlatModel:
    """What ``robust_dist_aggregate_`` / ``ServerOptimizer`` need of a model: a flat fp32 master."""

    def __init__(self, master):
        self.arena = types.SimpleNamespace(master=master, shadow=None)
        self.synced = 0

    def sync_shadow(self, force=False):
        self.synced += 1

    def mark_shadow_synced(self):
        self.synced += 1


def _states(M, n=2048, seed=0):
    """Honest clients at w + 1e-3 N(0, 1), w = 0.05 N(0, 1): the inputs the specification was tried on."""
    g = torch.Generator().manual_seed(seed)
    base = 0.05 * torch.randn(n, generator=g)
    return [base + 1e-3 * torch.randn(n, generator=g) for _ in range(M)]


def _f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _biteq(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ the specification
def test_pair_sqdist_equals_a_hand_written_loop():
    states = _states(4, n=48, seed=1)
    D = rd.torch_pair_sqdist(states)
    assert D.dtype == torch.float64 and D.shape == (4, 4)
    rows = [s.tolist() for s in states]
    for i in range(4):
        for j in range(4):
            want = math.fsum((a - b) * (a - b) for a, b in zip(rows[i], rows[j]))
            assert abs(float(D[i, j]) - want) <= 1e-14 * want, (i, j)
        assert float(D[i, i]) == 0.0
    assert torch.equal(D, D.t())
    # the difference first: two clients 1e-3 of their norm apart keep every digit (the Gram form
    # G_ii + G_jj - 2 G_ij in fp32 would not)
    a = torch.full((64,), 1.0)
    b = torch.full((64,), 1.0 + 2.0 ** -20)
    assert float(rd.torch_pair_sqdist([a, b])[0, 1]) == 64 * 2.0 ** -40
    with pytest.raises(ValueError, match="flat fp32"):
        rd.torch_pair_sqdist([a, b.double()])


def _hand_wmean(states, weights):
    M, n = len(states), states[0].numel()
    rows = [s.tolist() for s in states]
    w = [_f32(v) for v in weights]
    out = []
    for e in range(n):
        acc, first = 0.0, True
        for s in range(M):
            if w[s] == 0.0:
                continue
            t = _f32(w[s] * rows[s][e])
            acc = t if first else _f32(acc + t)
            first = False
        out.append(acc)
    dz = []
    for s in range(M):
        acc = 0.0
        for e in range(n):
            d = _f32(rows[s][e] - out[e])
            acc += _f32(d * d)
        dz.append(acc)
    return torch.tensor(out, dtype=torch.float32), dz


def test_weighted_mean_equals_a_hand_written_loop():
    states = _states(5, n=64, seed=2)
    for weights in ([0.2] * 5, [0.0, 0.5, 0.0, 0.25, 0.25], [0.0] * 5, [0.0, 0.0, 0.0, 0.0, 1.0],
                    [0.31, 0.07, 0.29, 0.02, 0.31]):
        out, Dz, nonfinite = rd.torch_weighted_mean_(states, weights)
        want, dz = _hand_wmean(states, weights)
        assert _biteq(out, want), weights
        assert Dz.dtype == torch.float64 and nonfinite == 0
        for a, b in zip(Dz.tolist(), dz):
            assert abs(a - b) <= 1e-12 * b, weights
    # no non-zero weight: +0, and the distances are the squared norms
    out, Dz, _ = rd.torch_weighted_mean_(states, [0.0] * 5)
    assert not out.view(torch.int32).any()
    assert Dz.tolist() == [float((s * s).double().sum()) for s in states]
    # the sum runs in slot order: the reverse order gives other bits
    w = [0.31, 0.07, 0.29, 0.02, 0.31]
    rev, _, _ = rd.torch_weighted_mean_(states[::-1], w[::-1])
    assert not _biteq(rev, rd.torch_weighted_mean_(states, w)[0])
    with pytest.raises(ValueError, match="weights"):
        rd.torch_weighted_mean_(states, [0.5, 0.5])


def test_zero_weight_nan_slot_and_pad():
    states = _states(4, n=128, seed=3)
    for s in states:
        s[32:96] = 0.0                                   # an alignment pad: +0 in every client
    states[2] = torch.full((128,), NAN)
    out, Dz, nonfinite = rd.torch_weighted_mean_(states, [0.5, 0.25, 0.0, 0.25])
    assert nonfinite == 0 and bool(torch.isfinite(out).all()) and math.isnan(float(Dz[2]))
    assert not out[32:96].view(torch.int32).any()
    out, _, nonfinite = rd.torch_weighted_mean_(states, [0.5, 0.25, 0.25, 0.0])
    assert nonfinite == 128
    states[2] = states[0].clone()
    r = rd.torch_multi_krum_(states, 0, 4)
    assert not r["out"][32:96].view(torch.int32).any() and r["flag"] == 0
    r = rd.torch_geometric_median_(states, 6, 1e-6)
    assert not r["out"][32:96].view(torch.int32).any() and r["flag"] == 0


# ------------------------------------------------------------------ krum_select
def _brute(D, f, m):
    """Scores by enumerating every neighbour subset of size c and taking the smallest sum; selection by
    enumerating every m-subset of the finite-score slots and taking the (total score, slots) minimum."""
    M = len(D)
    c = max(1, M - f - 2)
    clean = [[v if math.isfinite(v) else math.inf for v in row] for row in D]
    scores = []
    for i in range(M):
        others = [clean[i][j] for j in range(M) if j != i]
        scores.append(min(math.fsum(sub) for sub in itertools.combinations(others, c)))
    finite = [i for i in range(M) if math.isfinite(scores[i])]
    if len(finite) < m:
        return scores, None
    best = min(itertools.combinations(finite, m), key=lambda sub: (sorted(scores[i] for i in sub), sub))
    return scores, list(best)


@pytest.mark.parametrize("M", [3, 5, 8])
def test_krum_select_equals_a_brute_force_enumeration(M):
    states = _states(M, n=256, seed=10 + M)
    states[M - 1] = states[M - 1] * -4.0
    D = rd.torch_pair_sqdist(states)
    for f in range(0, max(1, (M - 3) // 2) + 1):
        for m in range(1, M - f + 1):
            scores, selected, weights, flag = rd.krum_select(D, f, m)
            want_scores, want_sel = _brute(D.tolist(), f, m)
            assert flag == 0 and selected == want_sel, (M, f, m)
            for a, b in zip(scores, want_scores):
                assert abs(a - b) <= 1e-15 * b, (M, f, m)
            assert weights == [_f32(1.0 / m) if i in selected else 0.0 for i in range(M)]
            if m <= M - 1:
                assert M - 1 not in selected             # the -4 x client is never among the closest
    assert rd.krum_select(D, 0, M)[1] == list(range(M))


def test_krum_select_tie_c_and_nonfinite():
    # equal scores: the lower slot
    D = [[0.0, 1.0, 1.0, 5.0], [1.0, 0.0, 1.0, 5.0], [1.0, 1.0, 0.0, 5.0], [5.0, 5.0, 5.0, 0.0]]
    scores, selected, weights, flag = rd.krum_select(D, 0, 1)       # c = 2
    assert scores == [2.0, 2.0, 2.0, 10.0] and selected == [0] and weights == [1.0, 0.0, 0.0, 0.0] and flag == 0
    assert rd.krum_select(D, 0, 2)[1] == [0, 1]
    assert rd.krum_select(D, 1, 3)[0] == [1.0, 1.0, 1.0, 5.0]       # c = 1
    # c = max(1, M - f - 2) at M = 2: each client's score is the distance to the other
    scores, selected, weights, flag = rd.krum_select([[0.0, 3.0], [3.0, 0.0]], 0, 2)
    assert scores == [3.0, 3.0] and selected == [0, 1] and weights == [0.5, 0.5]
    assert rd.krum_select([[0.0, 3.0], [3.0, 0.0]], 5, 1)[1] == [0]
    # ascending order of the sum: 1e16 + 1 + 1 in that order loses both ones
    big = [[0.0, 1e16, 1.0, 1.0], [1e16, 0.0, 1e16, 1e16], [1.0, 1e16, 0.0, 1.0], [1.0, 1e16, 1.0, 0.0]]
    assert rd.krum_select(big, 0, 1)[0][0] == 2.0 and rd.krum_select(big, 0, 1)[0][1] == 2e16
    # non-finite entries count as +inf
    inf = math.inf
    Dn = [[0.0, NAN, 1.0, 2.0], [NAN, 0.0, NAN, NAN], [1.0, NAN, 0.0, 1.5], [2.0, -inf, 1.5, 0.0]]
    scores, selected, weights, flag = rd.krum_select(Dn, 0, 3)      # c = 2
    assert scores == [3.0, inf, 2.5, 3.5] and selected == [0, 2, 3] and flag == 0
    scores, selected, weights, flag = rd.krum_select(Dn, 0, 2)
    assert scores[1] == inf and 1 not in selected and flag == 0
    # fewer than m finite scores: flag 1 and every weight 0
    Dbad = [[0.0, NAN, NAN], [NAN, 0.0, 1.0], [NAN, 1.0, 0.0]]
    scores, selected, weights, flag = rd.krum_select(Dbad, 0, 3)    # c = 1
    assert scores == [inf, 1.0, 1.0] and flag == 1 and selected == [] and weights == [0.0] * 3
    assert rd.krum_select(Dbad, 0, 2) == ([inf, 1.0, 1.0], [1, 2], [0.0, 0.5, 0.5], 0)
    for bad in ((Dbad, -1, 1), (Dbad, 0, 0), (Dbad, 0, 4), ([[0.0]], 0, 1)):
        with pytest.raises(ValueError, match="krum_select"):
            rd.krum_select(*bad)


def test_krum_params():
    assert [rd.default_byzantine(M) for M in (1, 2, 3, 4, 5, 8, 16)] == [0, 0, 0, 0, 1, 2, 6]
    assert rd.krum_params(8) == (2, 6) and rd.krum_params(8, None, 1) == (2, 1) and rd.krum_params(8, 1) == (1, 7)
    assert rd.krum_params(2) == (0, 2) and rd.krum_params(1) == (0, 1) and rd.krum_params(2, 0) == (0, 2)
    assert rd.krum_params(7, 2, 5) == (2, 5)
    with pytest.raises(ValueError, match="byzantine"):
        rd.krum_params(6, 2)                             # M < 2f + 3
    with pytest.raises(ValueError, match="byzantine"):
        rd.krum_params(6, -1)
    with pytest.raises(ValueError, match="krum_select"):
        rd.krum_params(8, 2, 7)                          # m > M - f
    with pytest.raises(ValueError, match="krum_select"):
        rd.krum_params(8, None, 0)


def test_multi_krum_scores_of_the_tried_inputs():
    """M = 8, f = 2, one -4 x client and one NaN client: honest scores about 0.016, the -4 x client's in
    the hundreds, the NaN client's inf."""
    states = _states(8, seed=3)
    states[3] = states[3] * -4.0
    states[5] = torch.full_like(states[5], NAN)
    r = rd.torch_multi_krum_(states, 2, 6)
    honest = [r["scores"][i] for i in (0, 1, 2, 4, 6, 7)]
    assert all(0.014 < s < 0.019 for s in honest) and 300 < r["scores"][3] < 800 and r["scores"][5] == math.inf
    assert r["selected"] == [0, 1, 2, 4, 6, 7] and r["flag"] == 0 and r["nonfinite"] == 0
    w = _f32(1 / 6)
    want, _, _ = rd.torch_weighted_mean_(states, [w, w, w, 0.0, w, 0.0, w, w])
    assert _biteq(r["out"], want) and bool(torch.isfinite(r["out"]).all())


def test_permutation_of_the_clients_permutes_the_weights():
    states = _states(6, seed=4)
    states[2] = states[2] * -4.0
    perm = [3, 0, 4, 2, 5, 1]
    shuffled = [states[p] for p in perm]
    a, b = rd.torch_multi_krum_(states, 1, 4), rd.torch_multi_krum_(shuffled, 1, 4)
    assert [b["weights"][perm.index(j)] for j in range(6)] == a["weights"] and a["weights"][2] == 0.0
    ga, gb = rd.torch_geometric_median_(states), rd.torch_geometric_median_(shuffled)
    for j in range(6):  # (the weighted sums run in another order: the weights agree to rounding, not to the bit)
        assert abs(gb["weights"][perm.index(j)] - ga["weights"][j]) <= 1e-5 * ga["weights"][j]
    assert min(range(6), key=lambda i: gb["weights"][i]) == perm.index(2)


# ------------------------------------------------------------------ Weiszfeld
def test_geomed_weights_mirror():
    beta, objective, flag, beta64 = rd.geomed_weights([4.0, 16.0, NAN, math.inf], 1e-6)
    assert beta64 == [(1 / 2) / (1 / 2 + 1 / 4), (1 / 4) / (1 / 2 + 1 / 4), 0.0, 0.0] and objective == 6.0 and flag == 0
    assert beta == [_f32(b) for b in beta64]
    assert rd.geomed_weights([0.0, 0.0], 1e-6) == ([0.5, 0.5], 0.0, 0, [0.5, 0.5])     # nu floors a distance
    assert rd.geomed_weights([1e-20, 1.0], 1e-6)[3] == [1e6 / (1e6 + 1.0), 1.0 / (1e6 + 1.0)]
    assert rd.geomed_weights([NAN, math.inf], 1e-6) == ([0.0, 0.0], 0.0, 1, [0.0, 0.0])
    for nu in (0.0, -1.0, NAN, math.inf):
        with pytest.raises(ValueError, match="geomed_nu"):
            rd.geomed_weights([1.0], nu)


def test_weiszfeld_approaches_the_median_on_collinear_points():
    direction = torch.zeros(64)
    direction[3], direction[17] = 0.6, 0.8                # a unit vector
    ts = [-2.0, -0.5, 0.25, 1.0, 40.0]                    # 1-D median 0.25; the mean is 7.75
    states = [direction * t for t in ts]
    r = rd.torch_geometric_median_(states, 60, 1e-9)
    t = float((r["out"] * direction).sum())
    assert abs(t - 0.25) < 1e-3 and float((r["out"] - direction * t).abs().max()) < 1e-6
    six = float((rd.torch_geometric_median_(states, 6, 1e-9)["out"] * direction).sum())
    assert abs(six - 0.25) < abs(7.75 - 0.25) / 10        # already far from the mean


CASES = (("M8", 8, {3: "scale"}), ("M16", 16, {2: "scale", 7: "scale", 11: "scale"}), ("M3", 3, {2: "scale"}),
         ("nan", 5, {2: "nan"}), ("huge", 5, {1: "huge", 4: "huge"}))


@pytest.mark.parametrize("name,M,liars", CASES, ids=[c[0] for c in CASES])
def test_weiszfeld_on_the_tried_inputs(name, M, liars):
    """6 iterations, nu = 1e-6: the objective is non-increasing from pass 1 on (relative slack 1e-6), a
    -4 x client ends below 0.1 / M, a NaN client and a client at 3e30 (its fp32 squares overflow) get
    exactly 0."""
    states = _states(M, seed=M)
    for j, kind in liars.items():
        states[j] = {"scale": states[j] * -4.0, "nan": torch.full_like(states[j], NAN),
                     "huge": torch.full_like(states[j], 3e30)}[kind]
    r = rd.torch_geometric_median_(states, 6, 1e-6)
    obj = r["objective"]
    assert r["flag"] == 0 and r["nonfinite"] == 0 and len(obj) == 7 and bool(torch.isfinite(r["out"]).all())
    assert all(obj[i + 1] <= obj[i] * (1 + 1e-6) for i in range(1, 6)), obj
    for j, kind in liars.items():
        if kind == "scale":
            assert 0.0 < r["weights"][j] < 0.1 / M, (name, r["weights"])
        else:
            assert r["weights"][j] == 0.0 and not math.isfinite(r["Dz"][j])
    assert abs(sum(r["weights"]) - 1.0) < 1e-6
    want, Dz, _ = rd.torch_weighted_mean_(states, r["weights"])
    assert _biteq(r["out"], want)
    honest = [i for i in range(M) if i not in liars]
    centre = torch.stack([states[i] for i in honest]).mean(dim=0)
    assert float((r["out"] - centre).norm()) < 0.05 * float((states[honest[0]] * 5).norm())
    if name == "M3":
        assert obj[6] < obj[5] < obj[4]                   # still falling at iteration 6
    with pytest.raises(ValueError, match="geomed_iters"):
        rd.torch_geometric_median_(states, 0)


def test_weiszfeld_fails_at_pass_zero_only():
    states = [torch.full((64,), NAN), torch.full((64,), 3e30), torch.full((64,), math.inf)]
    r = rd.torch_geometric_median_(states, 6, 1e-6)
    assert r["flag"] == 1 and r["out"] is None and len(r["objective"]) == 1


# ------------------------------------------------------------------ configuration
def test_names_and_refusals():
    assert rb.AGGREGATORS == ("mean", "trimmed_mean", "median", "multi_krum", "geometric_median")
    assert rd.DIST_AGGREGATORS == rb.DIST_AGGREGATORS == ("multi_krum", "geometric_median")
    cfg = config.FedConfig()
    assert (cfg.byzantine, cfg.krum_select, cfg.geomed_iters, cfg.geomed_nu) == (None, None, 6, 1e-6)
    for kind in rd.DIST_AGGREGATORS:
        assert rb.check_robust_config(config.FedConfig(aggregator=kind)) == kind
        with pytest.raises(ValueError, match="aggregator"):
            rb.trim_count(8, kind)                       # no trim count
        r = rb.make_robust(config.FedConfig(aggregator=kind, byzantine=1, krum_select=2, geomed_iters=3, geomed_nu=1e-4))
        assert (r.aggregator, r.byzantine, r.krum_select, r.geomed_iters, r.geomed_nu) == (kind, 1, 2, 3, 1e-4)
        for kw, match in ((dict(transport="tcp"), "transport"), (dict(weighted_fedavg=True), "weighted_fedavg"),
                          (dict(byzantine=-1), "byzantine"), (dict(krum_select=0), "krum_select"),
                          (dict(geomed_iters=0), "geomed_iters"), (dict(geomed_nu=0.0), "geomed_nu"),
                          (dict(geomed_nu=-1e-6), "geomed_nu"), (dict(geomed_nu=NAN), "geomed_nu"),
                          (dict(geomed_nu=math.inf), "geomed_nu")):
            with pytest.raises(ValueError, match=match):
                rb.check_robust_config(config.FedConfig(aggregator=kind, **kw))
    # the bare word stays refused, and says where Krum went
    with pytest.raises(ValueError, match="aggregator.*multi_krum.*krum_select=1"):
        rb.check_robust_config(config.FedConfig(aggregator="krum"))
    with pytest.raises(ValueError, match="aggregator"):
        rb.trim_count(8, "krum")
    # the plain mean ignores the new fields
    assert rb.check_robust_config(config.FedConfig(byzantine=-1, geomed_nu=0.0)) is None
    # compress and secagg keep refusing every aggregator but the mean
    cp = import_module(f"{PKG}.parallel.compress")
    sa = import_module(f"{PKG}.parallel.secagg")
    for kind in rd.DIST_AGGREGATORS:
        with pytest.raises(ValueError, match="aggregator"):
            cp.check_compress_config(config.FedConfig(aggregator=kind, compress="int8"), 1)
        with pytest.raises(ValueError, match="aggregator"):
            sa.check_secagg_config(config.FedConfig(aggregator=kind, secagg=True), 1, 3)


def _cfg(outdir, rounds, **kw):
    base = dict(out_dir=outdir, synthetic_rows=600, data_fraction=0.1, max_len=32, epochs=1, batch_size=8,
                eval_batch_size=16, plots=False, resume=False, rounds=rounds, verbose=False, heartbeat_s=0.0,
                save_checkpoints=False)
    base.update(kw)
    return config.FedConfig(**base)


def _client(cfg, frame):
    return runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1)).setup()


def test_config_env_and_cli_reach_the_runner(monkeypatch, tmp_path):
    parser = config.FedConfig.add_cli(argparse.ArgumentParser())
    cfg = config.FedConfig.from_args(parser.parse_args(
        ["--aggregator", "multi_krum", "--byzantine", "1", "--krum-select", "2", "--geomed-iters", "4",
         "--geomed-nu", "1e-5"]))
    assert (cfg.aggregator, cfg.byzantine, cfg.krum_select, cfg.geomed_iters, cfg.geomed_nu) == \
        ("multi_krum", 1, 2, 4, 1e-5)
    for k, v in (("FEDDDOS_AGGREGATOR", "geometric_median"), ("FEDDDOS_BYZANTINE", "2"), ("FEDDDOS_KRUM_SELECT", "3"),
                 ("FEDDDOS_GEOMED_ITERS", "9"), ("FEDDDOS_GEOMED_NU", "1e-3")):
        monkeypatch.setenv(k, v)
    cfg = config.FedConfig.from_args(parser.parse_args([]))
    assert (cfg.aggregator, cfg.byzantine, cfg.krum_select, cfg.geomed_iters, cfg.geomed_nu) == \
        ("geometric_median", 2, 3, 9, 1e-3)
    cfg = config.FedConfig.from_args(parser.parse_args(["--aggregator", "multi_krum", "--krum-select", "1"]))  # flags win
    assert (cfg.aggregator, cfg.byzantine, cfg.krum_select) == ("multi_krum", 2, 1)
    _clear_rank_env()
    for k, v in dict(out_dir=str(tmp_path), synthetic_rows=600, max_len=32, plots=False, resume=False, verbose=False,
                     heartbeat_s=0.0).items():
        setattr(cfg, k, v)
    client = _client(cfg, None)
    r = client.robust
    assert (r.aggregator, r.byzantine, r.krum_select, r.geomed_iters, r.geomed_nu) == ("multi_krum", 2, 1, 9, 1e-3)
    for k in ("FEDDDOS_AGGREGATOR", "FEDDDOS_BYZANTINE", "FEDDDOS_KRUM_SELECT", "FEDDDOS_GEOMED_ITERS",
              "FEDDDOS_GEOMED_NU"):
        monkeypatch.delenv(k)
    assert _client(_cfg(str(tmp_path), 1), None).robust is None
    # refused at setup, before any work
    for kw, match in ((dict(aggregator="krum"), "aggregator"), (dict(aggregator="multi_krum", transport="tcp"), "transport"),
                      (dict(aggregator="geometric_median", weighted_fedavg=True), "weighted_fedavg"),
                      (dict(aggregator="multi_krum", byzantine=-1), "byzantine"),
                      (dict(aggregator="multi_krum", krum_select=0), "krum_select"),
                      (dict(aggregator="geometric_median", geomed_iters=0), "geomed_iters"),
                      (dict(aggregator="geometric_median", geomed_nu=0.0), "geomed_nu"),
                      (dict(aggregator="multi_krum", compress="int8"), "aggregator"),
                      (dict(aggregator="geometric_median", secagg=True), "aggregator")):
        with pytest.raises(ValueError, match=match):
            _client(_cfg(str(tmp_path), 1, **kw), None)


def test_round_time_refusals_name_the_flag():
    states = _states(6, n=64, seed=6)
    model = FlatModel(torch.zeros(64))
    with pytest.raises(ValueError, match="byzantine=2 needs at least 2f \\+ 3 = 7"):
        rb.RobustAggregator("multi_krum", byzantine=2).aggregate_(model, states)
    with pytest.raises(ValueError, match="krum_select=6"):
        rb.RobustAggregator("multi_krum", byzantine=1, krum_select=6).aggregate_(model, states)
    with pytest.raises(ValueError, match="krum_select=6"):
        rb.RobustAggregator("multi_krum", krum_select=6).aggregate_(model, states)      # f = 1 of 6
    assert not model.arena.master.any() and model.synced == 0
    with pytest.raises(ValueError, match="no participating"):
        rb.RobustAggregator("geometric_median").aggregate_(model, [])
    with pytest.raises(ValueError, match="aggregator"):
        rd.robust_dist_aggregate_(model, states, "median")
    # the old kinds go where they went
    rep = rb.RobustAggregator("median").aggregate_(model, states)
    want, trimmed, _ = rb.torch_robust_(states, 2)
    assert torch.equal(model.arena.master, want) and rep["k"] == 2 and "kind" not in rep


# ------------------------------------------------------------------ the default path
class _NoNewFields:
    """A configuration as the parent commit knew it: the new fields do not exist."""

    def __init__(self, cfg):
        self.__dict__.update({f.name: getattr(cfg, f.name) for f in dataclasses.fields(cfg) if f.name not in NEW_FIELDS})

    def client_seed(self, client_id):
        return self.base_seed + client_id


def test_default_mean_and_median_are_untouched(tmp_path, monkeypatch):
    """2 clients x 1 round: ``aggregator="mean"`` against a configuration without the new fields never reaches
    the distance-based code; ``median`` neither, and its record and log line are what they were."""
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)

    def boom(*a, **k):
        raise AssertionError("the path reached the distance-based aggregate")

    monkeypatch.setattr(rd, "robust_dist_aggregate_", boom)

    def run(cfg, n=2):
        client = _client(cfg, frame)
        said = []
        res = runner.run_virtual_clients(client, n, rounds=1, progress=said.append)
        return client.model.arena.master.clone(), res, said

    cfg = _cfg(str(tmp_path), 1)
    old = _NoNewFields(cfg)
    assert not any(hasattr(old, f) for f in NEW_FIELDS)
    a, ra, said_a = _single_thread(lambda: run(cfg))
    b, rb_, said_b = _single_thread(lambda: run(old))
    assert torch.equal(a, b)
    strip = lambda lines: [ln.split(" (")[0] if "steps," in ln else ln for ln in lines]  # noqa: E731 (drop timings)
    assert strip(said_a) == strip(said_b) and not any("robust" in ln or "Krum" in ln for ln in said_a)
    assert "robust" not in ra["rounds"][0] and "trimmed_share" not in ra["rounds"][0]
    med, rm, said_m = _single_thread(lambda: run(_cfg(str(tmp_path), 1, aggregator="median"), 3))
    rec = rm["rounds"][0]
    assert rec["k"] == 1 and len(rec["trimmed_share"]) == 3 and "robust" not in rec
    line = [ln for ln in said_m if "robust aggregate" in ln]
    assert len(line) == 1 and line[0].startswith("round 1/1 robust aggregate of 3 client(s), k = 1: most trimmed is participant ")
    assert line[0].endswith("(honest expectation 0.6667)")


# ------------------------------------------------------------------ collective runs
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
    rep = client.report()
    torch.save({"master": client.model.arena.master.clone(), "history": client.history, "report": rep},
               os.path.join(outdir, f"state_rank{rank}.pt"))
    client.log.close()
    comm.shutdown()


@pytest.mark.parametrize("kind", ["multi_krum", "geometric_median"])
def test_virtual_run_equals_three_rank_gloo_run(kind, tmp_path):
    world, rounds = 3, 2
    real = tmp_path / "real"
    real.mkdir()
    kw = dict(aggregator=kind, krum_select=2)
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
    for s in st:
        assert torch.equal(s["master"], st[0]["master"])
    assert torch.equal(st[0]["master"], client.model.arena.master) and not torch.equal(init, st[0]["master"])
    for r in range(rounds):
        got = res["rounds"][r]["robust"]
        assert got["kind"] == kind and got["clients"] == 3
        if kind == "multi_krum":
            assert (got["f"], got["m"]) == (0, 2) and len(got["selected"]) == 2 and len(got["rejected"]) == 1
            assert len(got["distances"]) == 3 and got["distances"][1][1] == 0.0
        else:
            assert (got["iters"], got["nu"]) == (6, 1e-6) and len(got["objective"]) == 7
            assert abs(sum(got["weights"]) - 1.0) < 1e-6 and min(got["weights"]) > 0.1
        for rank in range(world):
            want = st[rank]["history"][r]
            assert want["robust"] == got and "trimmed_share" not in want, (rank, r)
            assert res["rounds"][r]["clients"][rank]["aggregated_test"]["loss"] == want["aggregated_test"]["loss"], (rank, r)
    # the last round's report is in federated_report.json
    assert st[0]["report"]["robust"] == res["rounds"][-1]["robust"]
    with open(real / "federated_report.json") as f:
        assert json.load(f)["robust"]["kind"] == kind


def _flat_worker(rank, world, port, outdir, drop_rank, kind, with_server):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    comm = import_module(f"{PKG}.parallel.comm")
    fedavg = import_module(f"{PKG}.parallel.fedavg")
    comm.init_distributed(device="cpu")
    mine = _states(world, n=256, seed=11)[rank]
    model = FlatModel(mine.clone())
    server = so.ServerOptimizer(FlatModel(torch.zeros(256)), "adam", lr=0.01) if with_server else None
    robust = rb.RobustAggregator(kind)
    total = fedavg.fedavg_(model, participate=rank != drop_rank, server=server, robust=robust)
    torch.save({"master": model.arena.master.clone(), "total": total, "last": robust.last,
                "synced": model.synced}, os.path.join(outdir, f"flat{rank}.pt"))
    comm.shutdown()


@pytest.mark.parametrize("kind", ["multi_krum", "geometric_median"])
def test_dropped_client(kind, tmp_path):
    """N = 4, client 3's update dropped: 3 rows enter, and the dropped client receives the same aggregate."""
    mp.spawn(_flat_worker, args=(4, _free_port(), str(tmp_path), 2, kind, False), nprocs=4, join=True)
    states = _states(4, n=256, seed=11)
    live = [states[0], states[1], states[3]]
    if kind == "multi_krum":
        r = rd.torch_multi_krum_(live, 0, 3)
    else:
        r = rd.torch_geometric_median_(live, 6, 1e-6)
    for rank in range(4):
        got = torch.load(tmp_path / f"flat{rank}.pt", weights_only=False)
        assert got["total"] == 3.0 and got["last"]["clients"] == 3 and got["last"]["kind"] == kind, rank
        assert torch.equal(got["master"], r["out"]) and got["synced"] == 1, rank
    _clear_rank_env()
    fedavg = import_module(f"{PKG}.parallel.fedavg")
    model = FlatModel(states[0].clone())                 # one process: one client is a copy
    assert fedavg.fedavg_(model, participate=True, robust=rb.RobustAggregator(kind)) == 1.0
    assert torch.equal(model.arena.master, states[0])
    assert fedavg.fedavg_(model, participate=False, robust=rb.RobustAggregator(kind)) == 0.0


# ------------------------------------------------------------------ a client that lies
def test_nan_poisoner_is_rejected_and_named_while_the_mean_goes_nan(tmp_path):
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    poison = dict(poison_client=1, poison_kind="nan")

    def run(**kw):
        client = _client(_cfg(str(tmp_path), 1, **poison, **kw), frame)
        said = []
        res = runner.run_virtual_clients(client, 3, rounds=1, progress=said.append)
        return client.model.arena.master.clone(), res, said

    mean, _, _ = _single_thread(lambda: run())
    assert not bool(torch.isfinite(mean).any())
    out, res, said = _single_thread(lambda: run(aggregator="multi_krum", krum_select=2))
    rep = res["rounds"][0]["robust"]
    assert bool(torch.isfinite(out).all()) and rep["rejected"] == [1] and rep["selected"] == [0, 2]
    assert rep["scores"][1] == math.inf and math.isnan(rep["distances"][1][0])
    assert any("multi-Krum of 3 client(s), f = 0, m = 2: rejected participant(s) 2 (score inf)" in ln for ln in said)
    out, res, said = _single_thread(lambda: run(aggregator="geometric_median"))
    rep = res["rounds"][0]["robust"]
    assert bool(torch.isfinite(out).all()) and rep["weights"][1] == 0.0 and abs(rep["weights"][0] - 0.5) < 0.2
    assert any("geometric median of 3 client(s), 6 iteration(s): lowest weight is participant 2 with 0.000000 "
               "(uniform 0.333333)" in ln for ln in said)


@pytest.mark.parametrize("kind", ["multi_krum", "geometric_median"])
def test_one_liar_too_many_raises_and_leaves_the_master(kind):
    n = 128
    states = [torch.full((n,), NAN) for _ in range(3)]
    if kind == "multi_krum":
        states[1] = _states(1, n=n, seed=5)[0]           # its only neighbours are NaN: no finite score
    start = _states(1, n=n, seed=6)[0]
    model = FlatModel(start.clone())
    srv = so.ServerOptimizer(FlatModel(torch.zeros(n)), "adam", lr=0.01)
    with pytest.raises(RuntimeError, match="left the model as it was: non-finite scores / distances at slot 0"):
        rd.robust_dist_aggregate_(model, states, kind, srv)
    assert torch.equal(model.arena.master, start) and model.synced == 0
    assert srv.rounds == 0 and not srv.m.any()
    # one inf entry makes a client's every distance inf: asking for all three finds only two
    if kind == "multi_krum":
        lied = _states(3, n=n, seed=7)
        lied[2][5] = math.inf
        with pytest.raises(RuntimeError, match="too few usable"):
            rd.robust_dist_aggregate_(model, lied, kind, None, 0, 3)


# ------------------------------------------------------------------ compositions
@pytest.mark.parametrize("kind", ["multi_krum", "geometric_median"])
def test_composes_with_server_adam(kind):
    n = 2048
    g = torch.Generator().manual_seed(9)
    x0 = 0.05 * torch.randn(n, generator=g)
    states = [x0 + 1e-3 * torch.randn(n, generator=g) for _ in range(5)]
    states[3] = states[3] * -4.0
    model = FlatModel(x0.clone())
    srv = so.ServerOptimizer(model, "adam", lr=0.01, betas=(0.9, 0.99), tau=1e-3)
    robust = rb.RobustAggregator(kind)
    rep = robust.aggregate_(model, states, srv)
    if kind == "multi_krum":
        assert rep["rejected"] == [3] and (rep["f"], rep["m"]) == (1, 4)
        agg = rd.torch_multi_krum_(states, 1, 4)["out"]
    else:
        assert 0.0 < rep["weights"][3] < 0.1 / 5
        agg = rd.torch_geometric_median_(states, 6, 1e-6)["out"]
    x, m = x0.clone(), torch.zeros(n)
    v = torch.full((n,), so.f32(so.f32(1e-3) * so.f32(1e-3)))
    d, dx = so.torch_chain_("adam", agg, x, m, v, 1.0, so.f32(0.01), so.f32(0.9), so.f32(0.99), so.f32(1e-3))
    assert torch.equal(model.arena.master, x) and torch.equal(srv.x, x)
    assert torch.equal(srv.m, m) and torch.equal(srv.v, v) and srv.rounds == 1
    assert srv.last["delta_l2"] == math.sqrt(float(d.double().square().sum()))
    assert model.synced == 1  # (the server step refreshes the shadow, once)
    model2 = FlatModel(x0.clone())
    rep2 = rb.RobustAggregator(kind).aggregate_(model2, states)
    assert torch.equal(model2.arena.master, agg) and model2.synced == 1 and repr(rep2) == repr(rep)


@pytest.mark.parametrize("kind", ["multi_krum", "geometric_median"])
def test_composes_with_privacy_clip(kind, tmp_path):
    """3 virtual clients with ``privacy_clip`` (no noise) and a -4 w poisoner: the clipped updates are
    aggregated, the poisoner (who lies after clipping) is rejected or weighted down, and the records carry
    both the privacy and the robust keys."""
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    cfg = _cfg(str(tmp_path), 1, aggregator=kind, krum_select=2, privacy_clip=0.05, privacy_seed=7, poison_client=2)

    def run():
        client = _client(cfg, frame)
        return client.model.arena.master.clone(), runner.run_virtual_clients(client, 3, rounds=1)

    out, res = _single_thread(run)
    rec = res["rounds"][0]
    assert bool(torch.isfinite(out).all()) and "privacy_epsilon" in rec and rec["robust"]["kind"] == kind
    assert all(c["clipped"] in (True, False) and c["update_l2"] > 0 for c in rec["clients"])
    if kind == "multi_krum":
        assert rec["robust"]["rejected"] == [2]
    else:
        assert rec["robust"]["weights"][2] < 0.1 / 3
