"""checkpoints.save_training_state / load_training_state: the reference's file names (base_trainer.py:183-202) holding state
dicts, pruning as :186-189, the resume pick (newest complete step), and the exact round trip of parameters, Adam moments,
scaler state, EMA and counters; load_generator reads the generator and EMA files written here."""
import importlib
import os

import pytest
import torch

ck = importlib.import_module("3dhumangan_amd.checkpoints")
ema_mod = importlib.import_module("3dhumangan_amd.lib.components.ema")


def _state(seed, steps=2):
    torch.manual_seed(seed)
    G, D = torch.nn.Sequential(torch.nn.Linear(4, 5), torch.nn.Linear(5, 3)), torch.nn.Linear(3, 2)
    G[0].bias.requires_grad_(False)                      # the EMA shadow list skips frozen parameters
    opt_g = torch.optim.Adam([{"params": [G[0].weight], "name": "generator", "lr": 1e-3},
                              {"params": list(G[1].parameters()), "name": "neural_field", "lr": 3e-3}], betas=(0.0, 0.9))
    opt_d = torch.optim.Adam(D.parameters(), lr=2e-3, betas=(0.0, 0.9), weight_decay=0.01)
    ema = ema_mod.ExponentialMovingAverage(G.parameters(), decay=0.999)
    scaler = torch.amp.GradScaler("cpu", init_scale=512.0, growth_interval=3)
    for _ in range(steps):
        for opt in (opt_g, opt_d):
            opt.zero_grad()
        D(G(torch.randn(6, 4))).square().mean().backward()
        opt_g.step()
        opt_d.step()
        ema.update(G.parameters())
    return dict(generator=G, discriminator=D, ema=ema, optimizer_G=opt_g, optimizer_D=opt_d, scaler=scaler)


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_round_trip_is_exact(tmp_path):
    a = _state(1)
    names = ck.save_training_state(str(tmp_path), 2000, epoch=3, seed=17, **a)
    assert sorted(names) == sorted(f"00002000_{k}.pth" for k in ck.TRAINING_FILES)
    assert sorted(os.listdir(tmp_path)) == sorted(names)                              # no temporary file left
    b = _state(2, steps=1)
    assert not _same(a["generator"].state_dict(), b["generator"].state_dict())
    rec = ck.load_training_state(str(tmp_path), **b)
    assert rec == {"step": 2000, "epoch": 3, "seed": 17}
    for k in ("generator", "discriminator", "optimizer_G", "optimizer_D", "scaler"):
        assert _same(a[k].state_dict(), b[k].state_dict()), k
    assert [g["name"] for g in b["optimizer_G"].param_groups] == ["generator", "neural_field"]
    assert _same(ck.ema_state(a["ema"]), ck.ema_state(b["ema"])) and b["ema"].num_updates == 2
    # the two runs continue identically
    for s in (a, b):
        torch.manual_seed(5)
        s["optimizer_G"].zero_grad()
        s["discriminator"](s["generator"](torch.randn(6, 4))).square().mean().backward()
        s["optimizer_G"].step()
        s["ema"].update(s["generator"].parameters())
    assert _same(a["generator"].state_dict(), b["generator"].state_dict()) and _same(ck.ema_state(a["ema"]), ck.ema_state(b["ema"]))


def test_files_hold_plain_data(tmp_path):
    """every file loads through torch's weights_only loader: state dicts, no pickled modules or classes of this package"""
    a = _state(1)
    for name in ck.save_training_state(str(tmp_path), 7, **a):
        obj = torch.load(os.path.join(tmp_path, name), weights_only=True)
        assert isinstance(obj, dict), name
    # the optimizer and scaler files are the reference's format: state_dict() as torch.save writes it
    assert _same(torch.load(os.path.join(tmp_path, "00000007_optimizer_G.pth"), weights_only=True), a["optimizer_G"].state_dict())
    assert _same(torch.load(os.path.join(tmp_path, "00000007_scaler.pth"), weights_only=True), a["scaler"].state_dict())


def test_pruning_and_the_resume_pick(tmp_path):
    a = _state(1)
    d = str(tmp_path)
    open(os.path.join(d, "notes.pth"), "w").close()                                   # not a step file: left alone
    for step in (1000, 2000, 3000):
        ck.save_training_state(d, step, keep_interval=2000, **a)
    assert ck.saved_steps(d) == [2000, 3000]                                          # 1000 pruned when 2000 was saved; 3000 is the newest
    assert not [n for n in os.listdir(d) if n.startswith("00001000")] and os.path.exists(os.path.join(d, "notes.pth"))
    os.remove(os.path.join(d, "00003000_trainer.pth"))                                # an interrupted save is not picked
    assert ck.load_training_state(d, **_state(3))["step"] == 2000
    with pytest.raises(FileNotFoundError):
        ck.load_training_state(d, step=3000, **_state(3))
    with pytest.raises(FileNotFoundError):
        ck.load_training_state(str(tmp_path / "empty"), **_state(3))
    a.pop("scaler")
    assert "00004000_scaler.pth" not in ck.save_training_state(d, 4000, **a)          # fp32 runs have no scaler file


def test_load_generator_reads_the_generator_and_ema_files(tmp_path):
    a = _state(1)
    ck.save_training_state(str(tmp_path), 5, **a)
    fresh = _state(9, steps=0)["generator"]
    fresh[0].bias.requires_grad_(False)
    ck.load_generator(fresh, str(tmp_path / "00000005_generator.pth"), ema_path=str(tmp_path / "00000005_ema.pth"))
    live = [p for p in fresh.parameters() if p.requires_grad]
    assert all(torch.equal(p, s) for p, s in zip(live, a["ema"].shadow_params))
    assert torch.equal(fresh[0].bias, a["generator"][0].bias)                         # frozen: from the generator file
    x = torch.randn(3, 4)
    a["ema"].store(a["generator"].parameters())
    a["ema"].copy_to(a["generator"].parameters())
    assert torch.equal(fresh(x), a["generator"](x))
