"""CPU: DDIMSampler.stochastic_encode / decode, the `timesteps=` subset of ddim_sampling and the runner's
image_guided_refinement - the PRODUCT sampler on the oracle's op table (oracle.ops_torch.TorchOps has no q_sample: the
sampler's torch expression runs) against tests/golden/ddim_small_partial.npz, recorded from the REAL reference's sampler at
base width 64 by tools/make_ddim_partial_golden.py.

Bounds: 5e-5 relative L2 for trajectories - the project's f32-vs-f32 bound for sampler fixtures (tests/test_oracle_golden.py);
bit equality for stochastic_encode (the same three f32 operations on the same f32 tables)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import golden_recipe as gr, ref_harness as rh
from oracle.ops_torch import TorchOps
from open_pandora_amd import synth, unet as U, wm
from open_pandora_amd.ddim import DDIMSampler
from open_pandora_amd.ddpm import LatentVisualDiffusion
from test_oracle_golden import RH_KW, load, rel

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
SHAPE = (1, 4, 16, 8, 8)
# key -> (model, S, eta, cfg, t_start): the fixture's cases (tools/make_ddim_partial_golden.py DECODE_CASES)
DECODE_CASES = {"v_S10_eta0_cfg4_t6": ("v", 10, 0.0, 4.0, 6), "v_S20_eta1_cfg4_t12": ("v", 20, 1.0, 4.0, 12),
                "eps_S10_eta0_cfg4_t6": ("eps", 10, 0.0, 4.0, 6)}
ENC_CASES = {"enc_t0": False, "enc_t9": False, "enc_b2_t2_7": False, "enc_orig_t0": True, "enc_orig_t999": True}
TRAJ_TOL = 5e-5


@functools.lru_cache(maxsize=None)
def golden():
    return load("ddim_small_partial.npz")


def product_model(which, ops):
    """The product shell at base width 64 on `ops`: "v" = the 512 / 1024 yaml's, "eps" = the 256 yaml's."""
    extra = gr.UNET_256_OVERRIDES if which == "eps" else {}
    m = U.UNetModel(**dict(RH_KW, model_channels=64, **extra)).eval()
    m.load_state_dict(synth.synth_state_dict(m, seed=gr.WEIGHT_SEED))
    if which == "eps":
        return LatentVisualDiffusion(m.bind(ops), parameterization="eps", rescale_betas_zero_snr=False,
                                     use_dynamic_rescale=False, image_size=(32, 32))
    return LatentVisualDiffusion(m.bind(ops))


@functools.lru_cache(maxsize=None)
def cpu_model(which):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return product_model(which, TorchOps())


class Spy:
    """Records the timestep and the keyword names of every apply_model call of a model, for the length of a `with`."""

    def __init__(self, pm):
        self.pm, self.steps, self.kwargs = pm, [], set()

    def __enter__(self):
        inner = self.pm.apply_model

        def logged(x, t, c, **kw):
            if not self.steps or self.steps[-1] != int(t[0]):
                self.steps.append(int(t[0]))
            self.kwargs |= set(kw)
            return inner(x, t, c, **kw)

        self.pm.apply_model = logged
        return self

    def __exit__(self, *exc):
        del self.pm.apply_model  # (the instance attribute: the class's method shows again)


def run_decode_case(pm, key, dev=lambda t: t, spy=True, **sampler_kw):
    """stochastic_encode -> decode of one fixture case on `pm` -> (z, out, visited timesteps; None without `spy`, whose
    host read of `t` cannot run inside a graph capture)."""
    g = golden()
    which, S, eta, cfg, t_start = DECODE_CASES[key]
    _, cond, uc = gr.sampler_inputs(8, 8)
    put = lambda c: {k: [dev(v) for v in lst] for k, lst in c.items()}
    ns = gr.noises(SHAPE, t_start)
    smp = DDIMSampler(pm, **sampler_kw)
    smp.make_schedule(S, "uniform_trailing", eta, verbose=False)
    z = smp.stochastic_encode(dev(torch.from_numpy(g[f"{key}/x0"])), torch.tensor([t_start - 1]),
                              noise=dev(torch.from_numpy(g[f"{key}/enc_noise"])))
    if not spy:
        return z, smp.decode(z, put(cond), t_start, cfg, put(uc), noise_fn=lambda i, shape: ns[i], verbose=False), None
    with Spy(pm) as log:
        y = smp.decode(z, put(cond), t_start, cfg, put(uc), noise_fn=lambda i, shape: ns[i], verbose=False)
    return z, y, log.steps


@pytest.mark.parametrize("key", list(DECODE_CASES))
def test_encode_then_decode_against_reference(key):
    g = golden()
    z, y, steps = run_decode_case(cpu_model(DECODE_CASES[key][0]), key)
    assert z.dtype == y.dtype == torch.float32
    assert np.array_equal(z.numpy(), g[f"{key}/z"])
    assert steps == g[f"{key}/timesteps"].tolist()
    assert np.isfinite(g[f"{key}/out"]).all()
    err = rel(y, g[f"{key}/out"])
    print(f"\n[parity] ddim partial {key} product sampler on the CPU op table: rel err {err:.2e}")
    assert err < TRAJ_TOL


def test_timesteps_subset_against_reference():
    """ddim_sampling(timesteps=6) after make_schedule(10): the reference's 5 steps (its off-by-one), the recorded timesteps,
    and `timesteps` no longer among the keywords that reach the U-Net."""
    g = golden()
    pm = cpu_model("v")
    ins, cond, uc = gr.sampler_inputs(8, 8)
    smp = DDIMSampler(pm)
    smp.make_schedule(10, "uniform_trailing", 0.0, verbose=False)
    with Spy(pm) as spy:
        y, _ = smp.ddim_sampling(cond, SHAPE, x_T=ins["x_T"], timesteps=6, unconditional_guidance_scale=4.0,
                                 unconditional_conditioning=uc, verbose=False, fs=torch.tensor([int(g["subset_fs"])]))
    assert spy.steps == g["v_S10_subset6/timesteps"].tolist() and len(spy.steps) == 5
    assert "timesteps" not in spy.kwargs and "ddim_use_original_steps" not in spy.kwargs and spy.kwargs == {"fs"}
    err = rel(y, g["v_S10_subset6/out"])
    print(f"\n[parity] ddim partial v_S10_subset6 product sampler on the CPU op table: rel err {err:.2e}")
    assert err < TRAJ_TOL


@pytest.mark.parametrize("key", list(ENC_CASES))
def test_stochastic_encode_bit_equal(key):
    g = golden()
    smp = DDIMSampler(cpu_model("v"))
    smp.make_schedule(10, "uniform_trailing", 0.0, verbose=False)
    out = smp.stochastic_encode(torch.from_numpy(g[f"{key}/x0"]), torch.from_numpy(g[f"{key}/t"]),
                                use_original_steps=ENC_CASES[key], noise=torch.from_numpy(g[f"{key}/noise"]))
    assert out.dtype == torch.float32 and np.array_equal(out.numpy(), g[f"{key}/out"])


def test_stochastic_encode_draws_its_noise_and_caches_its_tables():
    smp = DDIMSampler(cpu_model("v"))
    smp.make_schedule(10, "uniform_trailing", 0.0, verbose=False)
    x0 = torch.from_numpy(golden()["enc_t0/x0"])
    torch.manual_seed(3)
    a = smp.stochastic_encode(x0, torch.tensor([4]))
    tables = smp._encode_tables(False, smp._ops().device)
    torch.manual_seed(3)
    want = smp.stochastic_encode(x0, torch.tensor([4]), noise=torch.randn(x0.shape))
    assert torch.equal(a, want) and smp._encode_tables(False, smp._ops().device) is tables
    smp.make_schedule(20, "uniform_trailing", 0.0, verbose=False)  # a new schedule: new tables
    assert smp._encode_tables(False, smp._ops().device)[0].numel() == 20


def test_original_steps_loops_are_refused_and_the_reference_is_not_finite_there():
    g = golden()
    assert not bool(g["orig_steps_decode_finite"]) and not bool(g["orig_steps_decode_finite/v"])
    assert not bool(g["orig_steps_decode_finite/eps"])
    _, cond, uc = gr.sampler_inputs(8, 8)
    smp = DDIMSampler(cpu_model("v"))
    smp.make_schedule(10, "uniform_trailing", 0.0, verbose=False)
    z = torch.zeros(SHAPE)
    with pytest.raises(NotImplementedError, match="non-finite"):
        smp.decode(z, cond, 5, 4.0, uc, use_original_steps=True)
    with pytest.raises(NotImplementedError, match="non-finite"):
        smp.ddim_sampling(cond, SHAPE, x_T=z, ddim_use_original_steps=True, verbose=False)


def test_argument_checks():
    _, cond, uc = gr.sampler_inputs(8, 8)
    smp = DDIMSampler(cpu_model("v"))
    smp.make_schedule(10, "uniform_trailing", 0.0, verbose=False)
    z = torch.zeros(SHAPE)
    for t_start in (0, 11, -1):
        with pytest.raises(ValueError, match="t_start"):
            smp.decode(z, cond, t_start, 4.0, uc, verbose=False)
    for t, orig in (([10], False), ([-1], False), ([1000], True), ([-1], True)):
        with pytest.raises(ValueError, match="indices"):
            smp.stochastic_encode(z, torch.tensor(t), use_original_steps=orig, noise=z)
    with pytest.raises(ValueError, match="one per clip"):
        smp.stochastic_encode(z, torch.tensor([1, 2]), noise=z)


def test_multi_rank_and_multicond_samplers_refuse():
    from open_pandora_amd.ddim import DDIMSamplerMultiCond
    pm = cpu_model("v")
    z = torch.zeros(SHAPE)
    for smp in (DDIMSampler(pm, cfg_parallel=object()), DDIMSamplerMultiCond(pm)):
        smp.make_schedule(10, "uniform_trailing", 0.0, verbose=False)
        with pytest.raises(NotImplementedError):
            smp.stochastic_encode(z, torch.tensor([3]), noise=z)
        with pytest.raises(NotImplementedError):
            smp.decode(z, {}, 3, verbose=False)


def test_default_path_did_not_move():
    """ddim_sampling(timesteps=None) is sample()'s loop: equal bit for bit, and still the reference's trajectory."""
    S, eta, cfg = gr.DDIM_SMALL_CASES[0]
    want = load("ddim_small.npz")[f"S{S}_eta{eta:g}_cfg{cfg:g}"]
    pm = cpu_model("v")
    ins, cond, uc = gr.sampler_inputs(8, 8)
    kw = dict(unconditional_guidance_scale=cfg, unconditional_conditioning=uc, verbose=False, fs=torch.tensor([15]),
              x_T=ins["x_T"])
    smp = DDIMSampler(pm)
    a, _ = smp.sample(S=S, batch_size=1, shape=SHAPE[1:], conditioning=cond, eta=eta, timestep_spacing="uniform_trailing", **kw)
    smp2 = DDIMSampler(pm)
    smp2.make_schedule(S, "uniform_trailing", eta, verbose=False)
    b, _ = smp2.ddim_sampling(cond, SHAPE, timesteps=None, ddim_use_original_steps=False, **kw)
    assert torch.equal(a, b) and rel(a, want) < TRAJ_TOL


@pytest.mark.skipif(not rh.available(), reason="reference checkout not present")
def test_fixture_regenerates_from_the_live_reference():
    """One trajectory case and the original-steps quirk, regenerated from the reference checkout with the fixture's own tool."""
    sys.path.insert(0, TOOLS)
    try:
        import make_ddim_partial_golden as tool
    finally:
        sys.path.remove(TOOLS)
    g = golden()
    key = "v_S10_eta0_cfg4_t6"
    assert tool.DECODE_CASES == DECODE_CASES and int(g["x0_seed"]) == tool.X0_SEED
    rec = tool.run_decode_case(key)
    assert np.array_equal(rec["x0"], g[f"{key}/x0"]) and np.array_equal(rec["z"], g[f"{key}/z"])
    assert rec["timesteps"].tolist() == g[f"{key}/timesteps"].tolist()
    assert rel(rec["out"], g[f"{key}/out"]) < 1e-6  # (the same f32 program; thread counts may differ)
    assert tool.orig_steps_decode_finite("v") is False and not bool(g["orig_steps_decode_finite/v"])


# -- the runner ------------------------------------------------------------------------------------------------------------

def stub_runner(pm, decode_first_stage=None, dev=lambda t: t):
    """DiffusionRunner around `pm` with stub encoders: the image tokens of the recipe, a first stage that pools 8x8 (and
    records how many frames each call got)."""
    ins, _, _ = gr.sampler_inputs(8, 8)
    text, img = dev(ins["c_crossattn"][:, :77]), dev(ins["c_crossattn"][:, 77:])
    uct, uci = dev(ins["uc_crossattn"][:, :77]), dev(ins["uc_crossattn"][:, 77:])
    seen = []

    def encode(x, noise=None):
        seen.append(x.shape[0])
        p = torch.nn.functional.avg_pool2d(x.float(), 8)
        return 0.5 * torch.cat([p, p.mean(1, keepdim=True)], 1)

    run = wm.DiffusionRunner(pm, lambda im: img if float(im.abs().sum()) > 0 else uci, uct, encode, decode_first_stage)
    return run, text, seen


def hand_composition(run, text, videos, cond_image, z_init, t_enc, S, eta, cfg, fs, spacing, enc_noise, step_noises):
    """What image_guided_refinement is documented to do, written out."""
    z_cond = wm.get_latent_z(run.encode_first_stage, videos)
    img_emb, uc_img = run.embed_image(cond_image), run.embed_image(torch.zeros_like(cond_image))
    cond = {"c_crossattn": [torch.cat([text, img_emb], 1)], "c_concat": [z_cond]}
    uc = {"c_crossattn": [torch.cat([run.uncond_text_emb, uc_img], 1)], "c_concat": [z_cond]}
    smp = run.sampler
    smp.make_schedule(S, spacing, eta, verbose=False)
    z = smp.stochastic_encode(z_init, torch.full((z_init.shape[0],), t_enc - 1, dtype=torch.long), noise=enc_noise)
    return smp.decode(z, cond, t_enc, cfg, uc, fs=torch.tensor([fs] * z_init.shape[0], device=z_cond.device),
                      noise_fn=lambda i, shape: step_noises[i], verbose=False)


def test_runner_refinement_equals_the_hand_written_composition():
    pm = cpu_model("v")
    run, text, seen = stub_runner(pm)
    frame0 = gr.ae_pixels(1, 64, 64).permute(1, 0, 2, 3)[None]  # (1, 3, 1, 64, 64)
    cond_image = frame0[:, :, 0]
    z_init = gr.ae_latent(16, 8, 8)
    enc_noise, ns = torch.from_numpy(golden()["enc_t0/noise"]), gr.noises(SHAPE, 4)
    # (S = 20, eta 1, uniform_trailing: a schedule whose sigmas are finite on the v-model)
    kw = dict(ddim_steps=20, ddim_eta=1.0, unconditional_guidance_scale=4.0, fs=15, timestep_spacing="uniform_trailing")
    got = run.image_guided_refinement(text, frame0, cond_image, z_init, 0.1, encode_noise=enc_noise,
                                      noise_fn=lambda i, shape: ns[i], **kw)
    want = hand_composition(run, text, frame0, cond_image, z_init, 2, 20, 1.0, 4.0, 15, "uniform_trailing", enc_noise, ns)
    assert got.shape == (1, 1, 4, 16, 8, 8) and torch.equal(got[:, 0], want) and bool(torch.isfinite(got).all())
    assert seen == [1, 1]  # the conditioning frame, once per side; a latent `init` is not encoded


def test_runner_refinement_clamps_t_enc_chunks_the_encoder_and_decodes_frames():
    """strength 0 -> one step, strength 1 -> the whole schedule (spied: no U-Net run); 16 frames as `init` reach the first
    stage 4 at a time; `decode_first_stage` is applied per sample; the multi-condition sampler is refused."""
    pm = cpu_model("v")
    run, text, seen = stub_runner(pm, decode_first_stage=lambda z: z[:, :3].repeat_interleave(8, -1).repeat_interleave(8, -2))
    calls = []

    class SpySampler(DDIMSampler):
        def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
            calls.append(("enc", t.tolist(), tuple(x0.shape)))
            return x0

        def decode(self, x_latent, cond, t_start, *a, **k):
            calls.append(("dec", t_start, len(self.ddim_timesteps)))
            return x_latent

    run.sampler = SpySampler(pm)
    frame0 = gr.ae_pixels(1, 64, 64).permute(1, 0, 2, 3)[None]
    frames = gr.ae_pixels(16, 64, 64).permute(1, 0, 2, 3)[None]  # (1, 3, 16, 64, 64)
    kw = dict(ddim_steps=10, unconditional_guidance_scale=4.0, fs=15)
    for strength, t_enc in ((0.0, 1), (1.0, 10), (7.0, 10), (0.65, 6)):
        del calls[:], seen[:]
        out = run.image_guided_refinement(text, frame0, frame0[:, :, 0], frames, strength, n_samples=2, **kw)
        assert calls == [("enc", [t_enc - 1], (1, 4, 16, 8, 8)), ("dec", t_enc, 10)] * 2
        assert seen == [1, 4, 4, 4, 4] and out.shape == (1, 2, 3, 16, 64, 64)
    with pytest.raises(NotImplementedError, match="multi-condition"):
        run.image_guided_refinement(text, frame0, frame0[:, :, 0], frames, 0.5, multiple_cond_cfg=True, **kw)
    with pytest.raises(ValueError, match="init"):
        run.image_guided_refinement(text, frame0, frame0[:, :, 0], frames[:, :2], 0.5, **kw)


def test_world_model_forwards_refinement():
    from open_pandora_amd.model import WorldModel
    seen = {}

    class Runner:
        diffusion_model = None

        def image_guided_refinement(self, *a, **k):
            seen["a"], seen["k"] = a, k
            return "out"

    w = WorldModel(Runner(), None)
    assert w.image_guided_refinement("c", "v", "i", "init", 0.4, ddim_steps=7, fs=3, noise_fn=len) == "out"
    assert seen["a"] == ("c", "v", "i", "init", 0.4) and seen["k"]["ddim_steps"] == 7 and seen["k"]["noise_fn"] is len
    assert seen["k"]["fs"] == 3 and seen["k"]["n_samples"] == 1
