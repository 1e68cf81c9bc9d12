"""FedProx on the CPU (torch path): ArenaAdam's proximal term against ``p.grad += mu * (p - p0)``
followed by torch.optim, the anchor's life cycle, the --prox-mu / FEDDDOS_PROX_MU plumbing, the
``label_skew`` partition, and a 2-client x 2-round virtual run whose round-2 anchors are round 1's
aggregate."""
import argparse
import os

import numpy as np
import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd import data as data_pkg
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.config import FedConfig
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.data.dataset import (
    build_client_data, partition_rows)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.data.featurize import (
    clean_frame)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import ArenaAdam
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.fed import runner
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier, DistilBertConfig)

HF_NO_DECAY = ("bias", "LayerNorm", "layer_norm")
MU = 0.1


def small(layers=1, seed=0):
    return DDoSClassifier(config=DistilBertConfig(n_layers=layers), seed=seed)


def batch(B=4, S=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(999, 2000, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1:, S // 2:] = 0
    ids = ids * mask
    ids[:, 0] = 101
    return ids, mask, torch.randint(0, 2, (B,), generator=g)


def _no_decay(name):
    return any(s in name for s in HF_NO_DECAY)


def _run(model, opt, steps, torch_prox=None, sched=None):
    """``steps`` training steps on one batch.  torch_prox = (mu, {name: p0}): the reference arm --
    ``p.grad += mu * (p - p0)`` before every ``step()`` of a torch optimizer."""
    ids, mask, y = batch()
    model.train()
    for step in range(steps):
        model.torch_counter = step
        if torch_prox is None:
            opt.zero_grad()
        else:
            opt.zero_grad(set_to_none=False)
            model.zero_grad()
        loss, _ = model.forward_loss(ids, mask, y)
        loss.backward()
        if torch_prox is not None:
            mu, p0 = torch_prox
            with torch.no_grad():
                for n, p in model.named_parameters():
                    p.grad += mu * (p - p0[n])
        opt.step()
        if sched is not None:
            sched.step()
    return {k: v.clone() for k, v in model.state_dict().items()}


def _single_thread(fn):
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)  # (as tests/test_model_cpu.py: the GEMM reductions split by thread count)
    try:
        return fn()
    finally:
        torch.set_num_threads(nthreads)


def hf_linear(w, T):
    """HF get_linear_schedule_with_warmup's lambda, spelled out."""
    return lambda c: c / max(1, w) if c < w else max(0, (T - c) / max(1, T - w))


@pytest.mark.parametrize("kind", ["adam", "groups", "groups_linear"])
def test_prox_matches_torch(kind):
    """3 steps of ArenaAdam(prox_mu=0.1) against torch.optim.Adam (coupled decay 0.01) and
    torch.optim.AdamW with the HF no-decay group (constant rate, and under the linear schedule), the
    torch arms with ``p.grad += mu * (p - p0)`` before each step.  |diff| <= 1e-6."""
    sch_kw = dict(schedule="linear", warmup_steps=1, total_steps=4) if kind == "groups_linear" else {}

    def arms():
        m = small(seed=3)
        if kind == "adam":
            opt = ArenaAdam(m, lr=1e-3, weight_decay=0.01, prox_mu=MU)
        else:
            opt = ArenaAdam(m, lr=1e-3, weight_decay=0.01, decoupled=True, no_decay=HF_NO_DECAY, prox_mu=MU, **sch_kw)
        got = _run(m, opt, 3)
        r = small(seed=3)
        named = list(r.named_parameters())
        p0 = {n: p.detach().clone() for n, p in named}
        if kind == "adam":
            ropt = torch.optim.Adam(r.parameters(), lr=1e-3, weight_decay=0.01)
        else:
            ropt = torch.optim.AdamW(
                [{"params": [p for n, p in named if not _no_decay(n)], "weight_decay": 0.01},
                 {"params": [p for n, p in named if _no_decay(n)], "weight_decay": 0.0}], lr=1e-3)
        sched = torch.optim.lr_scheduler.LambdaLR(ropt, hf_linear(1, 4)) if sch_kw else None
        return got, _run(r, ropt, 3, torch_prox=(MU, p0), sched=sched), p0

    got, ref, p0 = _single_thread(arms)
    assert list(got) == list(ref)
    moved = 0.0
    for k in ref:
        if k.endswith("k_lin.bias"):
            # softmax is invariant to the key bias: its true gradient is 0 and Adam amplifies
            # round-off noise (|g| ~ 1e-10 << eps), so both runs move it by noise only
            # (tests/test_adamw_cpu.py makes the same exception).
            continue
        diff = (got[k] - ref[k]).abs().max().item()
        assert diff <= 1e-6, (k, diff)
        if k in p0:
            moved = max(moved, (ref[k] - p0[k]).abs().max().item())
    assert moved > 1e-4  # (the comparison is not between two models that stood still)


def test_prox_term_changes_the_step_and_mu_zero_is_bitwise_plain():
    def arms():
        out = {}
        for name, kw in (("plain", {}), ("zero", dict(prox_mu=0.0)), ("prox", dict(prox_mu=MU))):
            m = small(seed=3)
            opt = ArenaAdam(m, lr=1e-3, weight_decay=0.01, decoupled=True, no_decay=HF_NO_DECAY, **kw)
            _run(m, opt, 3)
            out[name] = (m.arena.master.clone(), opt.m.clone(), opt.v.clone(), opt)
        return out

    out = _single_thread(arms)
    for a, b in zip(out["plain"][:3], out["zero"][:3]):
        assert torch.equal(a, b)
    assert out["zero"][3].anchor is None and out["plain"][3].anchor is None
    assert "prox_mu" not in out["zero"][3].state_dict()
    assert not torch.equal(out["plain"][0], out["prox"][0])
    sd = out["prox"][3].state_dict()
    assert sd["prox_mu"] == MU and "anchor" not in sd


def test_prox_holds_the_model_near_its_anchor_and_reset_resnapshots():
    """6 identical steps from one seed: ||master - start|| is strictly smaller with mu = 1 than with
    mu = 0; the anchor is the start until reset_state() re-snapshots it, in place."""
    def arms():
        dist = {}
        for mu in (0.0, 1.0):
            m = small(seed=5)
            start = m.arena.master.clone()
            opt = ArenaAdam(m, lr=1e-3, prox_mu=mu)
            if mu:
                assert torch.equal(opt.anchor, start) and opt.anchor.data_ptr() != m.arena.master.data_ptr()
            _run(m, opt, 6)
            dist[mu] = (m.arena.master - start).norm().item()
            if mu:
                assert torch.equal(opt.anchor, start)  # steps never move it
                ptr = opt.anchor.data_ptr()
                opt.reset_state()
                assert torch.equal(opt.anchor, m.arena.master) and opt.anchor.data_ptr() == ptr
                assert not torch.equal(opt.anchor, start)
                assert int(opt.step_t.item()) == 0 and not opt.m.any() and not opt.v.any()
        return dist

    dist = _single_thread(arms)
    assert 0.0 < dist[1.0] < dist[0.0], dist


def test_prox_mu_reaches_the_runner_optimizer(monkeypatch):
    parser = FedConfig.add_cli(argparse.ArgumentParser())
    cfg = FedConfig.from_args(parser.parse_args(["--prox-mu", "0.05"]))
    assert cfg.prox_mu == 0.05
    m = small()
    opt = runner.make_optimizer(m, cfg)
    assert opt.prox_mu == 0.05 and torch.equal(opt.anchor, m.arena.master)
    assert opt.prox_args()[0] == 0.05 and opt.prox_args()[1] is opt.anchor
    # the teacher's optimizer takes no proximal term
    t_opt = runner.make_teacher_optimizer(small(), cfg)
    assert t_opt.prox_mu == 0.0 and t_opt.anchor is None and t_opt.prox_args() is None
    cfg.lr_schedule = "linear"
    t_opt = runner.make_teacher_optimizer(small(), cfg)
    assert t_opt.prox_mu == 0.0 and t_opt.anchor is None

    monkeypatch.setenv("FEDDDOS_PROX_MU", "0.25")
    cfg = FedConfig.from_env()
    assert cfg.prox_mu == 0.25 and runner.make_optimizer(small(), cfg).prox_mu == 0.25
    monkeypatch.delenv("FEDDDOS_PROX_MU")
    opt = runner.make_optimizer(small(), FedConfig())
    assert opt.prox_mu == 0.0 and opt.anchor is None and opt.prox_args() is None

    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="prox_mu"):
            ArenaAdam(small(), prox_mu=bad)
        with pytest.raises(ValueError, match="prox_mu"):
            runner.make_optimizer(small(), FedConfig(prox_mu=bad))


def test_prox_with_a_decaying_word_table_takes_the_dense_word_path():
    # decoupled decay of the word table alone keeps the sparse path (lazy row decay) ...
    m = small()
    ArenaAdam(m, weight_decay=0.01, decoupled=True, no_decay=HF_NO_DECAY)
    assert m.sparse_word_grad is True
    # ... with a proximal term a row without state drifts from its anchor: dense
    m = small()
    opt = ArenaAdam(m, weight_decay=0.01, decoupled=True, no_decay=HF_NO_DECAY, prox_mu=MU)
    assert opt.word_wd == 0.01 and m.sparse_word_grad is False and not opt.lazy_active()
    # word table in the no-decay group, or no decay at all: the sparse path as it is
    m = small()
    opt = ArenaAdam(m, weight_decay=0.01, decoupled=True, no_decay=("word_embeddings",), prox_mu=MU)
    assert opt.word_wd == 0.0 and m.sparse_word_grad is True
    m = small()
    ArenaAdam(m, prox_mu=MU)
    assert m.sparse_word_grad is True


# ------------------------------------------------------------------ label_skew partition
@pytest.fixture(scope="module")
def frame():
    return clean_frame(data_pkg.generate_cicids2017(3000, seed=0))


def _parent_rows(df, client_id, data_fraction, seed, partition, num_clients):
    """The row selection as it was before ``label_skew`` existed, written out."""
    if partition == "disjoint" and num_clients > 1:
        order = np.random.default_rng(0).permutation(len(df))
        df = df.iloc[order[client_id::num_clients]]
        frac = min(1.0, data_fraction * num_clients)
    else:
        frac = data_fraction
    return df.sample(frac=frac, random_state=seed)


def test_label_skew_shares_sizes_and_determinism(frame):
    for skew in (0.9, 0.5, 0.75):
        for v in range(4):
            seed = 42 + v
            iid = partition_rows(frame, v, 0.1, seed, "iid_overlap", 4)
            rows = partition_rows(frame, v, 0.1, seed, "label_skew", 4, skew)
            assert len(rows) == len(iid) == 300
            ddos = int((rows["Label"] == "DDoS").sum())
            want = (skew if v % 2 == 0 else 1.0 - skew) * len(rows)
            assert abs(ddos - want) <= 1.0, (skew, v, ddos, want)
            assert rows.index.is_unique  # sampled without replacement
            again = partition_rows(frame, v, 0.1, seed, "label_skew", 4, skew)
            assert list(again.index) == list(rows.index)
            other = partition_rows(frame, v, 0.1, seed + 100, "label_skew", 4, skew)
            assert list(other.index) != list(rows.index)
            # shuffled: the classes are not left back to back
            lab = (rows["Label"] == "DDoS").to_numpy()
            assert 1 < int(np.abs(np.diff(lab.astype(int))).sum())


def test_label_skew_errors(frame):
    for bad in (0.4, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="partition_skew"):
            partition_rows(frame, 0, 0.1, 42, "label_skew", 2, bad)
    n_ddos = int((frame["Label"] == "DDoS").sum())
    assert 0.95 * 0.9 * len(frame) > n_ddos  # (the request below cannot be met)
    with pytest.raises(ValueError, match="DDoS rows"):
        partition_rows(frame, 0, 0.9, 42, "label_skew", 2, 0.95)
    with pytest.raises(ValueError, match="benign rows"):
        partition_rows(frame, 1, 0.9, 43, "label_skew", 2, 0.95)


def test_iid_and_disjoint_partitions_are_unchanged(frame):
    for partition in ("iid_overlap", "disjoint"):
        for n_clients in (1, 3):
            for v in range(n_clients):
                got = partition_rows(frame, v, 0.1, 42 + v, partition, n_clients)
                ref = _parent_rows(frame, v, 0.1, 42 + v, partition, n_clients)
                assert list(got.index) == list(ref.index), (partition, n_clients, v)


def test_label_skew_client_data_keeps_the_split(frame):
    """build_client_data: label_skew draws as many rows as iid_overlap and splits them 60/20/20."""
    iid = build_client_data(frame, 0, 0.1, 42, 32, partition="iid_overlap", num_clients=2)
    skw = build_client_data(frame, 0, 0.1, 42, 32, partition="label_skew", num_clients=2, partition_skew=0.9)
    assert skw.n_rows == iid.n_rows == 300
    assert (len(skw.train), len(skw.val), len(skw.test)) == (len(iid.train), len(iid.val), len(iid.test)) == (180, 60, 60)
    total = int(skw.train.labels.sum() + skw.val.labels.sum() + skw.test.labels.sum())
    assert total == 270
    parser = FedConfig.add_cli(argparse.ArgumentParser())
    cfg = FedConfig.from_args(parser.parse_args(["--partition", "label_skew", "--partition-skew", "0.8"]))
    assert (cfg.partition, cfg.partition_skew) == ("label_skew", 0.8) and FedConfig().partition_skew == 0.9


# ------------------------------------------------------------------ virtual run
def test_virtual_run_anchors_each_round_at_the_last_aggregate(tmp_path, monkeypatch):
    """2 clients x 2 rounds on the label_skew partition with prox_mu = 0.01: every optimizer's anchor
    is the weights its round started from -- the shared init in round 1, round 1's aggregate in
    round 2, bit for bit -- and the final weights differ from the mu = 0 run."""
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    frame = data_pkg.generate_cicids2017(600, seed=0)
    opts, aggs = [], []
    make, average = runner.make_optimizer, runner._average_masters

    def spy_make(model, cfg, *a, **kw):
        opts.append(make(model, cfg, *a, **kw))
        return opts[-1]

    def spy_average(model, states):
        average(model, states)
        aggs.append(model.arena.master.detach().clone())

    monkeypatch.setattr(runner, "make_optimizer", spy_make)
    monkeypatch.setattr(runner, "_average_masters", spy_average)

    def run(mu):
        cfg = FedConfig(out_dir=str(tmp_path / f"mu{mu}"), synthetic_rows=600, data_fraction=0.1, max_len=32,
                        epochs=1, batch_size=8, eval_batch_size=16, plots=False, resume=False, rounds=2,
                        verbose=False, heartbeat_s=0.0, save_checkpoints=False, partition="label_skew",
                        partition_skew=0.9, prox_mu=mu)
        client = runner.FederatedClient(cfg, frame=frame, model_config=DistilBertConfig(n_layers=1)).setup()
        init = client.model.arena.master.detach().clone()
        del opts[:], aggs[:]
        res = runner.run_virtual_clients(client, 2, rounds=2)
        return res, init, client.model.arena.master.detach().clone()

    def both():
        res, init, final = run(0.01)
        assert len(opts) == 4 and len(aggs) == 2  # (round 1: clients 1, 2; round 2: clients 1, 2)
        for o in opts:
            assert o.prox_mu == 0.01
        assert torch.equal(opts[0].anchor, init) and torch.equal(opts[1].anchor, init)
        assert torch.equal(opts[2].anchor, aggs[0]) and torch.equal(opts[3].anchor, aggs[0])
        assert not torch.equal(aggs[0], init) and torch.equal(final, aggs[1])
        shares = [c["l2_local_to_start"] for r in res["rounds"] for c in r["clients"]]
        assert len(shares) == 4 and all(s > 0 for s in shares)
        _, init0, final0 = run(0.0)
        assert all(o.anchor is None for o in opts)
        assert torch.equal(init0, init) and not torch.equal(final0, final)

    _single_thread(both)
