"""Learning-rate schedules on the CPU (torch path): ArenaAdam's host mirror ``lr_at`` against
torch's LambdaLR with HF's lambdas, a scheduled AdamW run against torch.optim.AdamW + LambdaLR, the
configuration / train_model / federated-runner plumbing, the state_dict round trip and the refusals."""
import argparse
import os

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.config import FedConfig
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, train_model)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.fed import runner
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier, DistilBertConfig)

HF_NO_DECAY = ("bias", "LayerNorm", "layer_norm")
BASE_RATES = (2e-5, 3e-4, 1e-3)
GRID = ((0, 7), (3, 10), (1, 2), (5, 5), (4, 6), (100, 1272), (127, 3816))
# three fp32 roundings (the base rate, the divide, the multiply), each <= 2^-24, plus one to spare
REL_BOUND = 4 * 2.0 ** -24


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


def hf_linear(w, T):
    """HF get_linear_schedule_with_warmup's lambda, spelled out."""
    return lambda c: c / max(1, w) if c < w else max(0, (T - c) / max(1, T - w))


def hf_constant_with_warmup(w):
    return lambda c: c / max(1, w) if c < w else 1.0


def lambda_lr_table(base, lam, n):
    """The rates torch's LambdaLR hands optimizer steps 1..n (fp64)."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return out


def check_against_reference(got, ref, what):
    for t, (g, r) in enumerate(zip(got, ref), start=1):
        if r == 0.0:
            assert g == 0.0, (what, t, g)
        else:
            assert abs(g - r) <= REL_BOUND * abs(r), (what, t, g, r, abs(g - r) / abs(r))


@pytest.fixture(scope="module")
def model():
    return small()


@pytest.mark.parametrize("kind", ["linear", "constant_with_warmup"])
def test_lr_at_matches_lambda_lr(model, kind):
    opt = ArenaAdam(model, schedule=kind, warmup_steps=0, total_steps=7)
    worst = 0.0
    for base in BASE_RATES:
        opt.lr = base
        for w, T in GRID:
            opt.set_schedule(total_steps=T, warmup_steps=w)
            ref = lambda_lr_table(base, hf_linear(w, T) if kind == "linear" else hf_constant_with_warmup(w), T + 2)
            got = [opt.lr_at(t) for t in range(1, T + 3)]
            check_against_reference(got, ref, (kind, base, w, T))
            worst = max([worst] + [abs(g - r) / abs(r) for g, r in zip(got, ref) if r != 0.0])
            # fp32 values, as the device holds them
            assert all(g == float(torch.tensor(g, dtype=torch.float32)) for g in got)
    print(f"{kind}: worst relative error {worst:.3e} (bound {REL_BOUND:.3e})")
    if kind == "linear":
        opt.set_schedule(total_steps=10, warmup_steps=3)
        assert opt.lr_at(1) == 0.0 and opt.lr_at(11) == 0.0 and opt.lr_at(12) == 0.0  # the first step of a warmup: 0
    # step_offset shifts the ramp
    opt.set_schedule(total_steps=10, warmup_steps=3, step_offset=0)
    plain = [opt.lr_at(t) for t in range(1, 11)]
    opt.set_schedule(step_offset=4)
    assert [opt.lr_at(t) for t in range(1, 7)] == plain[4:]


def _no_decay(name):
    return any(s in name for s in HF_NO_DECAY)


def _run(model, opt, steps, sched=None, after_step=None):
    ids, mask, y = batch()
    model.train()
    for step in range(steps):
        model.torch_counter = step
        if sched is None:
            opt.zero_grad()
        else:
            opt.zero_grad(set_to_none=False)
            model.zero_grad()
        loss, _ = model.forward_loss(ids, mask, y)
        loss.backward()
        opt.step()
        if sched is not None:
            sched.step()
        if after_step is not None:
            after_step(step + 1)
    return {k: v.clone() for k, v in model.state_dict().items()}


def test_scheduled_adamw_matches_torch_and_stops_at_total():
    """8 steps of linear (3, 8) AdamW 0.01 with the HF no-decay group against torch.optim.AdamW (two
    groups) + LambdaLR, at the tolerance tests/test_adamw_cpu.py uses for its AdamW comparison; a
    ninth step, past ``total``, runs at rate 0: the parameters stay put while m and v still move."""
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        m = small(seed=3)
        opt = ArenaAdam(m, lr=1e-3, schedule="linear", warmup_steps=3, total_steps=8, weight_decay=0.01,
                        decoupled=True, no_decay=HF_NO_DECAY)
        got = _run(m, opt, 8)
        master8, m8, v8 = m.arena.master.clone(), opt.m.clone(), opt.v.clone()
        ids, mask, y = batch()
        m.torch_counter = 8
        opt.zero_grad()
        loss, _ = m.forward_loss(ids, mask, y)
        loss.backward()
        opt.step()
        assert opt.lr_at(9) == 0.0
        assert torch.equal(m.arena.master, master8)
        assert not torch.equal(opt.m, m8) and not torch.equal(opt.v, v8)

        r = small(seed=3)
        named = list(r.named_parameters())
        ropt = torch.optim.AdamW(
            [{"params": [p for n, p in named if not _no_decay(n)], "weight_decay": 0.01},
             {"params": [p for n, p in named if _no_decay(n)], "weight_decay": 0.0}], lr=1e-3)
        ref = _run(r, ropt, 8, sched=torch.optim.lr_scheduler.LambdaLR(ropt, hf_linear(3, 8)))
    finally:
        torch.set_num_threads(nthreads)
    assert list(got) == list(ref)
    for k in ref:
        if k.endswith("k_lin.bias"):  # (a true gradient of 0: both runs move it by round-off noise only)
            continue
        assert torch.allclose(got[k], ref[k], atol=1e-6, rtol=1e-5), k


def test_config_flags_and_env_reach_the_optimizer(monkeypatch):
    parser = FedConfig.add_cli(argparse.ArgumentParser())
    ns = parser.parse_args(["--lr-schedule", "linear", "--warmup-ratio", "0.1"])
    cfg = FedConfig.from_args(ns)
    assert (cfg.lr_schedule, cfg.warmup_ratio, cfg.warmup_steps, cfg.lr_schedule_scope) == ("linear", 0.1, 0, "round")
    opt = runner.make_optimizer(small(), cfg)
    assert opt.schedule == "linear" and opt.schedule_unresolved()
    opt.set_schedule(total_steps=25)
    assert opt.sched_args() == (1, 3, 25, 0)  # ceil(0.1 * 25) warmup steps
    ns = parser.parse_args(["--lr-schedule", "constant_with_warmup", "--warmup-ratio", "0.5", "--warmup-steps", "4",
                            "--lr-schedule-scope", "run"])
    cfg = FedConfig.from_args(ns)
    opt = runner.make_optimizer(small(), cfg, round_index=1, rounds=3, steps_per_round=10)
    assert opt.sched_args() == (2, 4, 30, 10)  # warmup_steps wins over the ratio; round 1 starts at 10
    teacher_opt = runner.make_teacher_optimizer(small(), cfg)
    assert teacher_opt.schedule == "constant_with_warmup" and teacher_opt.schedule_unresolved()

    monkeypatch.setenv("FEDDDOS_LR_SCHEDULE", "linear")
    monkeypatch.setenv("FEDDDOS_WARMUP_STEPS", "7")
    monkeypatch.setenv("FEDDDOS_LR_SCHEDULE_SCOPE", "run")
    cfg = FedConfig.from_env()
    assert (cfg.lr_schedule, cfg.warmup_steps, cfg.lr_schedule_scope) == ("linear", 7, "run")
    opt = runner.make_optimizer(small(), cfg, round_index=0, rounds=2, steps_per_round=20)
    assert opt.sched_args() == (1, 7, 40, 0)
    cfg.lr_schedule_scope = "epoch"
    with pytest.raises(ValueError, match="scope"):
        runner.make_optimizer(small(), cfg)


def test_defaults_are_the_constant_schedule():
    m = small()
    opt = runner.make_optimizer(m, FedConfig())
    assert opt.schedule == "constant" and opt.sched_args() is None and opt.lr_at(5) == opt.lr
    assert set(opt.state_dict()) == {"m", "v", "step", "lr", "betas", "eps", "weight_decay", "decoupled"}
    assert set(ArenaAdam(m).state_dict()) == set(opt.state_dict())
    t_opt = runner.make_teacher_optimizer(m, FedConfig())
    assert t_opt.schedule == "constant" and t_opt.weight_decay == 0.0 and t_opt.lr == FedConfig().lr


def test_train_model_resolves_the_total():
    ids, mask, y = batch()
    loader = [{"input_ids": ids, "attention_mask": mask, "labels": y} for _ in range(3)]
    m = small()
    opt = ArenaAdam(m, schedule="linear", warmup_ratio=0.5)
    tr = train_model(m, loader, None, opt, num_epochs=2, use_graph=False)
    assert tr["steps"] == 6 and opt.total_steps == 6 and opt.sched_args() == (1, 3, 6, 0)
    m = small()
    opt = ArenaAdam(m, schedule="linear", warmup_steps=1)
    tr = train_model(m, loader, None, opt, num_epochs=2, use_graph=False, max_steps=4)
    assert tr["steps"] == 4 and opt.total_steps == 4
    # a total given by the caller is left alone
    m = small()
    opt = ArenaAdam(m, schedule="linear", total_steps=50)
    train_model(m, loader, None, opt, num_epochs=1, use_graph=False, max_steps=1)
    assert opt.total_steps == 50


def test_scope_run_offsets_the_second_virtual_round(tmp_path, monkeypatch):
    """Scope "run": round r of a virtual run trains with step_offset = r * steps_per_round over a
    total of rounds * steps_per_round (the training itself is stubbed out: plumbing only)."""
    from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd import data
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    cfg = FedConfig(out_dir=str(tmp_path), synthetic_rows=600, data_fraction=0.1, max_len=64, epochs=2,
                    batch_size=8, eval_batch_size=32, plots=False, resume=False, rounds=2, verbose=False,
                    heartbeat_s=0.0, save_checkpoints=False, lr_schedule="linear", warmup_steps=2,
                    lr_schedule_scope="run")
    frame = data.generate_cicids2017(cfg.synthetic_rows, seed=0)
    client = runner.FederatedClient(cfg, frame=frame, model_config=DistilBertConfig(n_layers=1)).setup()
    seen = []

    def fake_train(model, loader, criterion, opt, epochs, **kw):
        seen.append((opt.sched_args(), epochs * len(loader)))
        return {"epoch_losses": [0.0], "steps": 0, "seconds": 0.0, "batches_per_sec": 0.0, "graph": False,
                "graph_error": None}

    monkeypatch.setattr(runner, "train_model", fake_train)
    runner.run_virtual_clients(client, 1, rounds=2)
    assert len(seen) == 2
    spr = seen[0][1]
    assert spr > 0 and seen[1][1] == spr
    assert seen[0][0] == (1, 2, 2 * spr, 0)
    assert seen[1][0] == (1, 2, 2 * spr, spr)
    # scope "round": the total is left to train_model, no offset
    open_ = []

    def fake_train_round(model, loader, criterion, opt, epochs, **kw):
        open_.append((opt.schedule, opt.schedule_unresolved(), opt.step_offset))
        opt.set_schedule(total_steps=epochs * len(loader))
        return fake_train(model, loader, criterion, opt, epochs)

    cfg.lr_schedule_scope = "round"
    monkeypatch.setattr(runner, "train_model", fake_train_round)
    runner.run_virtual_clients(client, 1, rounds=2)
    assert open_ == [("linear", True, 0), ("linear", True, 0)]


def test_state_dict_round_trip_resumes_the_ramp():
    """Saving after step 4 of 8 and loading into a fresh optimizer, then steps 5-8, equals the
    uninterrupted run bit for bit."""
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        kw = dict(lr=1e-3, schedule="linear", warmup_steps=3, total_steps=8, weight_decay=0.01, decoupled=True,
                  no_decay=HF_NO_DECAY)
        m = small(seed=3)
        whole = _run(m, ArenaAdam(m, **kw), 8)

        m = small(seed=3)
        opt = ArenaAdam(m, **kw)
        _run(m, opt, 4)
        sd = opt.state_dict()
        assert sd["schedule"] == {"name": "linear", "warmup_steps": 3, "warmup_ratio": 0.0, "total_steps": 8,
                                  "step_offset": 0}
        fresh = ArenaAdam(m, lr=1e-3, weight_decay=0.01, decoupled=True, no_decay=HF_NO_DECAY)
        assert fresh.schedule == "constant"
        fresh.load_state_dict(sd)
        assert fresh.sched_args() == (1, 3, 8, 0) and fresh.host_step == 4
        ids, mask, y = batch()
        for step in range(4, 8):
            m.torch_counter = step
            fresh.zero_grad()
            loss, _ = m.forward_loss(ids, mask, y)
            loss.backward()
            fresh.step()
    finally:
        torch.set_num_threads(nthreads)
    resumed = m.state_dict()
    assert list(resumed) == list(whole)
    for k in whole:
        assert torch.equal(resumed[k], whole[k]), k


def test_refusals():
    m = small()
    with pytest.raises(ValueError, match="unknown lr schedule"):
        ArenaAdam(m, schedule="cosine")
    with pytest.raises(ValueError, match="warmup_steps"):
        ArenaAdam(m, schedule="linear", warmup_steps=-1, total_steps=10)
    with pytest.raises(ValueError, match="warmup_steps"):
        ArenaAdam(m, schedule="linear", warmup_steps=11, total_steps=10)
    with pytest.raises(ValueError):
        ArenaAdam(m, schedule="linear", total_steps=10, step_offset=-1)
    with pytest.raises(ValueError):
        ArenaAdam(m, lr=float("inf"))
    ids, mask, y = batch()
    # step() with an unresolved total
    opt = ArenaAdam(m, schedule="linear", warmup_steps=2)
    m.train()
    opt.zero_grad()
    loss, _ = m.forward_loss(ids, mask, y)
    loss.backward()
    with pytest.raises(RuntimeError, match="total_steps"):
        opt.step()
    # set_schedule after a step
    opt.set_schedule(total_steps=5)
    opt.step()
    with pytest.raises(RuntimeError, match="taken a step"):
        opt.set_schedule(total_steps=9)
    opt.reset_state()
    opt.set_schedule(total_steps=9, step_offset=3)
    assert opt.sched_args() == (1, 2, 9, 3)
    with pytest.raises(ValueError):
        opt.set_schedule(warmup_steps=10)
    # the per-layer fused dW launches take a plain rate: a scheduled optimizer's hyper-parameters are refused
    from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine.optim import (
        FusedHyper)
    from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import (
        kernels as K)
    hp = FusedHyper([1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0])
    K._no_sched(hp, "linear_dw")
    hp.sched = opt.sched_args()
    with pytest.raises(ValueError, match="schedule"):
        K._no_sched(hp, "linear_dw")
