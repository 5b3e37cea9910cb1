"""The trainer's control plane on the CPU (lib/trainers/phase_trainer.py): the schedule against the values captured from the
reference (tests/golden/trainer_schedule.json, make_golden_trainer.py), every refusal by name, per-step seeding across a
resume, what is saved / pruned / logged, and a world-2 gloo run.  The networks are stand-ins (tests/_trainer_stubs.py); the two
step functions are the real discriminator_step / generator_step."""
import importlib
import json
import os
import socket

import pytest
import torch

from _trainer_stubs import GOLDEN, StubD, StubG, StubPreprocessor, StubSource, curriculum, stub_meta_over, stub_opt

pt = importlib.import_module("3dhumangan_amd.lib.trainers.phase_trainer")
trainers = importlib.import_module("3dhumangan_amd.lib.trainers")
ck = importlib.import_module("3dhumangan_amd.checkpoints")

SCHEDULE = json.load(open(os.path.join(GOLDEN, "trainer_schedule.json")))


def _norm(v):
    return json.loads(json.dumps(v))


def test_schedule_matches_the_reference():
    cur = curriculum()
    opt_g = torch.optim.Adam([{"params": [torch.nn.Parameter(torch.zeros(1))], "name": n} for n in SCHEDULE["groups"]], lr=1.0)
    opt_d = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    assert len(SCHEDULE["steps"]) == 20
    for s, want in SCHEDULE["steps"].items():
        at = pt.schedule(cur, int(s))
        if want.get("ended"):
            assert at is None, s
            continue
        meta, phase, alpha, noise = at
        assert _norm({k: v for k, v in meta.items()}) == want["meta"], s
        assert (phase, alpha, noise) == (want["phase"], want["alpha"], want["nerf_noise"]), s
        pt.set_learning_rate(opt_g, opt_d, meta)
        got = {g["name"]: g["lr"] for g in opt_g.param_groups} | {"discriminator": opt_d.param_groups[0]["lr"]}
        assert got == want["lrs"], s
        for g in opt_g.param_groups + opt_d.param_groups:
            assert list(g["betas"]) == want["betas"] and g["weight_decay"] == want["weight_decay"]
    # the fixture covers what it is meant to: two learning rates, a render-size raise, the fade, every phase, the end
    live = [v for v in SCHEDULE["steps"].values() if not v.get("ended")]
    assert len({v["lrs"]["generator"] for v in live}) == 2 and len({v["meta"]["render_height"] for v in live}) == 2
    assert {v["phase"] for v in live} == {0, 1, 2, 3} and 0 < min(v["alpha"] for v in live if v["alpha"] > 0) < 1


def test_unknown_group_name_is_refused():
    opt_g = torch.optim.Adam([{"params": [torch.nn.Parameter(torch.zeros(1))], "name": "mapping_network"}], lr=1.0)
    with pytest.raises(ValueError, match="param_group not defined"):
        pt.set_learning_rate(opt_g, torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1.0), pt.schedule(curriculum(), 0)[0])


@pytest.mark.parametrize("change, bs_factor, match", [
    (dict(batch_split=2), 1, "batch_split"), ({}, 2, "bs_factor"), (dict(ada_interval=4), 1, "ada_interval"),
    (dict(dual_discrimination=True), 1, "dual_discrimination"), ("uncond", 1, "uncond=False"), ("gen_modal", 1, "gen_modal")])
def test_refusals_by_name(tmp_path, change, bs_factor, match):
    cur = curriculum(**stub_meta_over())
    if change == "uncond":
        cur["phases"][2]["uncond"] = False
    elif change == "gen_modal":
        cur["phases"][1]["gen_modal"] = "rgbs_render"
    elif "batch_split" in change:
        cur[0]["batch_split"] = 2
    else:
        cur.update(change)
    with pytest.raises(ValueError, match=match):
        pt.PhaseTrainer(0, 1, "cpu", stub_opt(tmp_path, bs_factor=bs_factor), cur, StubSource(), generator=StubG(), discriminator=StubD(),
                        preprocessor=StubPreprocessor())


def _trainer(out, records=None, rank=0, world=1, **opt):
    torch.manual_seed(11)
    G, D = StubG(), StubD()
    return pt.PhaseTrainer(rank, world, "cpu", stub_opt(out, **opt), curriculum(**stub_meta_over()), StubSource(), generator=G,
                           discriminator=D, preprocessor=StubPreprocessor(), on_step=None if records is None else records.append)


def _same_record(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_run_steps_logs_and_ends_with_the_curriculum(tmp_path):
    rec = []
    t = _trainer(tmp_path, rec, log_interval=5).run()
    assert t.step == 15 and [r["step"] for r in rec] == list(range(15))                 # batch_size disappears at step 15
    assert [r["phase"] for r in rec] == [s % 4 for s in range(15)]
    assert [r["alpha"] for r in rec[:5]] == [0.0, 0.25, 0.5, 0.75, 1]
    assert rec[6]["lrs"][0] == 1e-4 and rec[8]["lrs"][0] == 5e-5                        # set per epoch: 8 items / batch 4 = 2 steps
    assert all(r["d_labels"] == r["g_labels"] == "rasterized_segments" for r in rec if r["phase"] in (1, 2))
    assert {r["d_labels"] for r in rec} == {"rasterized_segments", "body_segments"}
    assert t.source.asked[:4] == [(4, 0), (4, 1), (4, 2), (4, 3)]
    lines = [json.loads(ln) for ln in open(tmp_path / "train_log.jsonl")]
    assert [ln["step"] for ln in lines] == [0, 5, 10]
    assert set(lines[0]) == {"step", "epoch", "phase", "alpha", "lrs", "scale", "d", "g"} and set(lines[0]["lrs"]) == set(SCHEDULE["groups"]) | {"discriminator"}
    assert all(isinstance(v, float) and v == v for ln in lines for v in list(ln["d"].values()) + list(ln["g"].values()))
    assert ck.saved_steps(str(tmp_path)) == [15] and t.ema.num_updates == 15


def test_a_resumed_run_draws_what_the_uninterrupted_run_drew(tmp_path):
    whole, first, second = [], [], []
    a = _trainer(tmp_path / "a", whole, max_steps=6).run()
    _trainer(tmp_path / "b", first, max_steps=3).run()
    b = _trainer(tmp_path / "b", second, max_steps=6)
    assert b.step == 3 and b.epoch == 1                                                 # picked up from the directory
    b.run()
    assert [r["step"] for r in first + second] == list(range(6))
    for x, y in zip(whole, first + second):
        _same_record(x, y)                                                              # z, views, phase, lrs, alpha, noise, label choice
    for k in ("generator", "discriminator", "optimizer_G", "optimizer_D"):
        sa, sb = getattr(a, k).state_dict(), getattr(b, k).state_dict()
        assert str(sa) == str(sb), k
    assert all(torch.equal(x, y) for x, y in zip(a.ema.shadow_params, b.ema.shadow_params))
    with pytest.raises(ValueError, match="seed"):
        _trainer(tmp_path / "b", seed=4)
    assert not torch.equal(whole[1]["z_d"], whole[2]["z_d"]) and not torch.equal(whole[1]["z_d"], whole[1]["z_g"])
    assert not torch.equal(whole[1]["d_view"], whole[1]["g_view"])                       # a rotate phase: two draws of the view


def test_saving_interval_and_pruning(tmp_path):
    t = _trainer(tmp_path, save_interval=2, model_keep_interval=4, max_steps=7).run()
    assert t.step == 7
    # saved before steps 2, 4, 6 and at the end (7); each save first removes steps that are no multiple of 4
    assert ck.saved_steps(str(tmp_path)) == [4, 7]
    assert sorted({n[:8] for n in os.listdir(tmp_path) if n.endswith(".pth")}) == ["00000004", "00000007"]
    assert _trainer(tmp_path).step == 7


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, out, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rec = []
        t = _trainer(out, rec, rank=rank, world=world, max_steps=4).run()
        w = torch.cat([p.detach().flatten() for p in list(t.generator.parameters()) + list(t.discriminator.parameters())])
        q.put((rank, [r["step"] for r in rec], [r["phase"] for r in rec], t.source.asked, w.tolist(), rec[1]["z_d"].tolist(), None))
    except Exception:
        import traceback
        q.put((rank, None, None, None, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_world2_gloo_same_steps_and_only_rank0_writes(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, str(tmp_path / f"rank{r}"), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=120) for _ in procs), key=lambda g: g[0])
    for p in procs:
        p.join(timeout=60)
    for g in got:
        assert g[6] is None, g[6]
    assert got[0][1] == got[1][1] == [0, 1, 2, 3] and got[0][2] == got[1][2]
    assert got[0][3] == [(2, 0), (2, 2), (2, 4), (2, 6)] and got[1][3] == [(2, 1), (2, 3), (2, 5), (2, 7)]     # batch 4 // 2, own shards
    assert got[0][4] == got[1][4]                      # the gradient all-reduce keeps the ranks' weights identical
    assert got[0][5] != got[1][5]                  # each rank draws its own z
    assert ck.saved_steps(str(tmp_path / "rank0")) == [4] and os.path.exists(tmp_path / "rank0" / "train_log.jsonl")
    assert not os.path.exists(tmp_path / "rank1") or not os.listdir(tmp_path / "rank1")
