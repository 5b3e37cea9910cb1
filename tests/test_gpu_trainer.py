"""PhaseTrainer on the GPU with real networks: a tiny Map3DGenerator (the configuration of tests/golden/gen_train_mixed.npz) and
a two-block UNetDiscriminator at 16 x 8, synthetic.SyntheticTrainingSource with 8 bodies, batch 2, fp32.
 (a) run() over a 4-phase list with one do_r1 and one rotate phase; (b) save after 2 steps, resume: the loaded state is the saved
 state and step 2 sees bit-identical inputs; (c) load_generator on the written generator + EMA files reproduces the trainer's
 EMA generator; (d) the fused segmentation loss inside the steps against the torch loss, bar as in tests/test_gpu_seg_loss.py."""
import importlib
import json
import types

import pytest
import torch

from _seg_loss_reference import seg_loss_f64, ulp32
from conftest import load_golden

pytestmark = pytest.mark.gpu
pt = importlib.import_module("3dhumangan_amd.lib.trainers.phase_trainer")
losses = importlib.import_module("3dhumangan_amd.lib.trainers.losses")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
ck = importlib.import_module("3dhumangan_amd.checkpoints")
gens = importlib.import_module("3dhumangan_amd.lib.generators")
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")


def _curriculum():
    cur = {k: v for k, v in load_golden("gen_train_mixed")["meta"].items() if k not in ("nerf_noise",)}
    phases = [dict(name="uncond", uncond=True, gen_modal="rgbs", rotate=r, do_r1=d)
              for r, d in zip((False, True, False, False), (False, False, True, False))]
    cur.update({0: dict(batch_size=2, batch_split=1, gen_lr=1e-4, disc_lr=4e-4), 1000: {}}, phases=phases, betas=(0, 0.9),
               neural_field_cls="COORDCONCATSIREN", discriminator_blocks=2, use_mixed_precision=False, fade_steps=2)
    return cur


def _opt(out, **over):
    opt = types.SimpleNamespace(output_dir=str(out), n_epochs=100, seed=5, save_interval=1000, model_keep_interval=1000, log_interval=1,
                                max_steps=None, bs_factor=1)
    for k, v in over.items():
        setattr(opt, k, v)
    return opt


def _trainer(out, records=None, seg_loss=None, **over):
    source = synthetic.SyntheticTrainingSource(length=8, gen_height=16, gen_width=8, seed=1)
    return pt.PhaseTrainer(0, 1, "cuda", _opt(out, **over), _curriculum(), source, seg_loss=seg_loss,
                           on_step=None if records is None else records.append)


def _states(t):
    return [t.generator.state_dict(), t.discriminator.state_dict(), t.optimizer_G.state_dict(), t.optimizer_D.state_dict(),
            ck.ema_state(t.ema)]


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_source_is_a_learnable_toy_task():
    src = synthetic.SyntheticTrainingSource(length=8, gen_height=16, gen_width=8, seed=1)
    a, b = src.batches(2, 3, "cuda"), src.batches(2, 3, "cuda")
    assert a["images"].shape == (2, 3, 16, 8) and a["body_segments"].shape == (2, 16, 8) and a["body_segments"].dtype == torch.int64
    assert all(torch.equal(a[k], b[k]) for k in a) and a["indices"].tolist() == [6, 7]
    assert float(a["images"].abs().max()) <= 1 and int(a["body_segments"].max()) > 1 and int(a["body_segments"].max()) < 26
    clean = src.palette.cuda()[a["body_segments"]].permute(0, 3, 1, 2)
    assert float((a["images"] - clean).abs().max()) < 0.2                       # the palette of the labels plus a little noise


def test_run_four_steps_over_four_phases(tmp_path):
    rec = []
    t = _trainer(tmp_path, rec, max_steps=4).run()
    assert t.step == 4 and t.ema.num_updates == 4 and [r["phase"] for r in rec] == [0, 1, 2, 3]
    lines = [json.loads(ln) for ln in open(tmp_path / "train_log.jsonl")]
    assert [ln["step"] for ln in lines] == [0, 1, 2, 3] and [ln["alpha"] for ln in lines] == [0.0, 0.5, 1, 1]
    for ln in lines:
        assert all(v == v and abs(v) < 1e6 for v in list(ln["d"].values()) + list(ln["g"].values())), ln
    # gan_lambda = 0: the R1 target softmax(.).sum() is constant per pixel, so the penalty is rounding noise (>= 0)
    assert lines[2]["d"]["r1"] >= 0 and lines[0]["d"]["r1"] == 0 and all(ln["d"]["segmentation"] > 0 for ln in lines)
    assert rec[1]["d_labels"] == rec[1]["g_labels"] == "rasterized_segments"
    assert not torch.equal(rec[1]["d_view"], rec[1]["g_view"]) and torch.equal(rec[0]["d_view"], rec[0]["g_view"])
    assert ck.saved_steps(str(tmp_path)) == [4]


def test_resume_loads_the_saved_state_and_repeats_the_draws(tmp_path):
    whole, first, second = [], [], []
    _trainer(tmp_path / "a", whole, max_steps=3).run()
    a = _trainer(tmp_path / "b", first, max_steps=2).run()
    b = _trainer(tmp_path / "b", second, max_steps=3)
    assert b.step == 2 and _same(_states(a), _states(b))
    b.run()
    assert [r["step"] for r in second] == [2]
    x, y = whole[2], second[0]
    assert x.keys() == y.keys()
    for k in x:
        assert torch.equal(x[k], y[k]) if torch.is_tensor(x[k]) else x[k] == y[k], k


def test_load_generator_reproduces_the_ema_generator(tmp_path):
    t = _trainer(tmp_path, max_steps=2).run()
    meta = {k: v for k, v in pt.schedule(_curriculum(), 0)[0].items() if isinstance(k, str)}
    kw = dict(meta, neural_field_cls=impl.COORDCONCATSIREN, nerf_noise=0)
    fresh = gens.Map3DGenerator(**kw).cuda()
    ck.load_generator(fresh, str(tmp_path / "00000002_generator.pth"), ema_path=str(tmp_path / "00000002_ema.pth"), map_location="cuda")
    fresh.set_device("cuda")
    t.ema.copy_to(t.generator.parameters())
    data = t.preprocessor(t.source.batches(2, 0, "cuda"), False, **meta)
    z = torch.randn(2, meta["latent_dim"], generator=torch.Generator().manual_seed(1)).cuda()
    outs = []
    for G in (t.generator.eval(), fresh.eval()):
        torch.manual_seed(9)
        with torch.no_grad():
            outs.append(G(z, data, **kw)["rgbs"])
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_fused_loss_in_the_steps_against_the_torch_loss(tmp_path):
    calls = {"fused": [], "torch": []}

    def recording(name, fn):
        def call(segments, gt, label_dim, prior, mode):
            out = fn(segments, gt, label_dim, prior, mode)
            calls[name].append((segments.detach().clone(), gt.clone(), float(out[0].detach().double())))
            return out
        return call

    logs = {}
    for name, fn in (("torch", losses.segmentation_loss), ("fused", losses.segmentation_loss_fused)):
        _trainer(tmp_path / name, seg_loss=recording(name, fn), max_steps=1).run()
        logs[name] = json.loads(open(tmp_path / name / "train_log.jsonl").readline())
    assert len(calls["fused"]) == len(calls["torch"]) == 3                      # D on real, D on fake, the G step
    for i, (segments, gt, got) in enumerate(calls["fused"]):
        want = seg_loss_f64(segments.float().cpu().numpy(), gt.cpu().numpy(), None)["loss"]
        e_ref = abs(float(losses.segmentation_loss(segments.float(), gt, segments.shape[1])[0].double()) - want)
        print(f"call {i}: loss {want:.9f} err {abs(got - want):.3e} e_ref {e_ref:.3e}")
        assert abs(got - want) <= max(4 * e_ref, 4 * ulp32(want)), (i, got, want, e_ref)
    # the D step sees identical logits in both runs (same state, same draws): its scalar differs by the two losses' errors only
    d_f, d_t = logs["fused"]["d"]["segmentation"], logs["torch"]["d"]["segmentation"]
    assert torch.equal(calls["fused"][0][0], calls["torch"][0][0])
    assert abs(d_f - d_t) <= 16 * ulp32(d_t), (d_f, d_t)
    # the G step follows a D update that differs in the last bits: 1e-4, as in tests/test_gpu_seg_loss_step.py
    assert abs(logs["fused"]["g"]["segmentation"] - logs["torch"]["g"]["segmentation"]) <= 1e-4 * abs(logs["torch"]["g"]["segmentation"])
