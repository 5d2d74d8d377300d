"""Writes tests/golden/ddim_small_partial.npz: the REAL reference's img2img pair - DDIMSampler.stochastic_encode
(ddim.py:314-328) and DDIMSampler.decode (:292-312) - and the `timesteps=` subset of ddim_sampling (:161-165), on the real
LatentVisualDiffusion at base width 64 (weights gr.WEIGHT_SEED, inputs gr.sampler_inputs(8, 8)), f32 on the CPU.  The
reference is imported through oracle.ref_harness; `noise_like` is replaced by the recipe's seeded draws (gr.noises), as
oracle/make_golden.py does; the clip that is noised and the encode noise come from the seeded generators below and are
recorded.  Data only: inputs that are not recipe-derived, outputs, the timesteps the U-Net was called at.

  <case>/x0, /enc_noise, /z, /out, /timesteps    stochastic_encode(x0, [t_start - 1]) -> decode(z, cond, t_start, cfg, uc)
  v_S10_subset6/out, /timesteps                  ddim_sampling(cond, shape, x_T, timesteps=6) after make_schedule(10)
  enc_*/x0, /noise, /t, /out                     stochastic_encode alone (DDIM tables and the 1000-entry original tables)
  orig_steps_decode_finite[/v, /eps]             is decode(..., 5, use_original_steps=True) finite in the reference?

    python tools/make_ddim_partial_golden.py
"""
import contextlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from oracle import golden_recipe as gr  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from open_pandora_amd import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ddim_small_partial.npz")
X0_SEED, ENC_NOISE_SEED = 20240314, 20240315
SHAPE = (1, 4, 16, 8, 8)
SPACING = "uniform_trailing"
SUBSET_FS = 15  # ddim_sampling takes fs; decode does not (the U-Net's default_fs applies there)

# key -> (model, S, eta, cfg, t_start)
DECODE_CASES = {"v_S10_eta0_cfg4_t6": ("v", 10, 0.0, 4.0, 6), "v_S20_eta1_cfg4_t12": ("v", 20, 1.0, 4.0, 12),
                "eps_S10_eta0_cfg4_t6": ("eps", 10, 0.0, 4.0, 6)}
SUBSET_CASE = ("v_S10_subset6", "v", 10, 0.0, 4.0, 6)  # 5 steps: the reference's off-by-one (ddim.py:164)
# key -> (batch, t, use_original_steps), after make_schedule(10)
ENC_CASES = {"enc_t0": (1, [0], False), "enc_t9": (1, [9], False), "enc_b2_t2_7": (2, [2, 7], False),
             "enc_orig_t0": (1, [0], True), "enc_orig_t999": (1, [999], True)}


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def clip_and_noise(batch=1):
    shape = (batch,) + SHAPE[1:]
    return 0.7 * seeded(shape, X0_SEED), seeded(shape, ENC_NOISE_SEED)


_MODELS = {}


def reference_model(which):
    """The real LatentVisualDiffusion at base width 64: "v" = the 512 / 1024 shell, "eps" = the 256 yaml's (as gen_ddim_eps)."""
    if which not in _MODELS:
        if which == "v":
            m = rh.reference_diffusion(dict(model_channels=64))
        else:
            import yaml
            with open(os.path.join(rh.REFERENCE_ROOT, "DynamiCrafter", "configs", "inference_256_v1.0.yaml")) as f:
                kw = yaml.safe_load(f)["model"]["params"]["unet_config"]["params"]
            m = rh.reference_diffusion(dict(kw, model_channels=64, use_checkpoint=False), shell=gr.SHELL_256)
            assert m.parameterization == "eps" and not m.use_dynamic_rescale
        m.model.diffusion_model.load_state_dict(synth.synth_state_dict(m.model.diffusion_model, seed=gr.WEIGHT_SEED))
        _MODELS[which] = m
    return _MODELS[which]


@contextlib.contextmanager
def recipe_noise(nsteps):
    """The reference sampler's `noise_like` replaced by the recipe's seeded draws, for the length of the block."""
    import lvdm.models.samplers.ddim as refddim
    noises = iter(gr.noises(SHAPE, nsteps))
    real, refddim.noise_like = refddim.noise_like, lambda shape, device, repeat=False: next(noises)
    try:
        yield
    finally:
        refddim.noise_like = real


def _sampler(m, S, eta):
    """-> (sampler after make_schedule, list the visited timesteps are appended to)"""
    smp = rh.reference_sampler(m)
    smp.make_schedule(S, SPACING, eta, verbose=False)
    visited = []
    inner = m.apply_model

    def logged(x, t, c, **kw):
        if not visited or visited[-1] != int(t[0]):
            visited.append(int(t[0]))
        return inner(x, t, c, **kw)

    smp.model = _Logged(m, logged)
    return smp, visited


class _Logged:
    """The model with apply_model wrapped: every other attribute is the real model's."""

    def __init__(self, m, apply_model):
        self.__dict__.update(_m=m, apply_model=apply_model)

    def __getattr__(self, k):
        return getattr(self._m, k)


@torch.no_grad()
def run_decode_case(key):
    which, S, eta, cfg, t_start = DECODE_CASES[key]
    _, cond, uc = gr.sampler_inputs(8, 8)
    smp, visited = _sampler(reference_model(which), S, eta)
    x0, noise = clip_and_noise()
    z = smp.stochastic_encode(x0, torch.tensor([t_start - 1]), noise=noise)
    with recipe_noise(t_start):
        out = smp.decode(z, cond, t_start, cfg, uc)
    return {"x0": x0.numpy(), "enc_noise": noise.numpy(), "z": z.float().numpy(), "out": out.float().numpy(),
            "timesteps": np.asarray(visited, np.int64)}


@torch.no_grad()
def run_subset_case():
    key, which, S, eta, cfg, k = SUBSET_CASE
    ins, cond, uc = gr.sampler_inputs(8, 8)
    smp, visited = _sampler(reference_model(which), S, eta)
    with recipe_noise(S):
        out, _ = smp.ddim_sampling(cond, SHAPE, x_T=ins["x_T"], timesteps=k, unconditional_guidance_scale=cfg,
                                   unconditional_conditioning=uc, verbose=False, fs=torch.tensor([SUBSET_FS]))
    return {"out": out.float().numpy(), "timesteps": np.asarray(visited, np.int64)}


@torch.no_grad()
def run_enc_case(key):
    batch, t, orig = ENC_CASES[key]
    smp, _ = _sampler(reference_model("v"), 10, 0.0)
    x0, noise = clip_and_noise(batch)
    out = smp.stochastic_encode(x0, torch.tensor(t), use_original_steps=orig, noise=noise)
    return {"x0": x0.numpy(), "noise": noise.numpy(), "t": np.asarray(t, np.int64), "out": out.float().numpy()}


@torch.no_grad()
def orig_steps_decode_finite(which):
    """The reference's own decode(..., 5, use_original_steps=True): sigma of index 0 is 0 / 0 on the bf16 buffers."""
    _, cond, uc = gr.sampler_inputs(8, 8)
    smp, _ = _sampler(reference_model(which), 10, 0.0)
    x0, noise = clip_and_noise()
    z = smp.stochastic_encode(x0, torch.tensor([4]), use_original_steps=True, noise=noise)
    with recipe_noise(5):
        out = smp.decode(z, cond, 5, 4.0, uc, use_original_steps=True)
    return bool(torch.isfinite(out).all())


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {"x0_seed": np.int64(X0_SEED), "enc_noise_seed": np.int64(ENC_NOISE_SEED), "subset_fs": np.int64(SUBSET_FS)}
    recorded = []

    def put(key, rec):
        for k, v in rec.items():
            out[f"{key}/{k}"] = v
        recorded.append((key, rec["out"]))
        print(f"{key}: {time.time() - t0:.1f}s std {rec['out'].std():.4f}"
              + (f" timesteps {rec['timesteps'].tolist()}" if "timesteps" in rec else ""), flush=True)

    for key in DECODE_CASES:
        t0 = time.time()
        put(key, run_decode_case(key))
    t0 = time.time()
    put(SUBSET_CASE[0], run_subset_case())
    for key in ENC_CASES:
        t0 = time.time()
        put(key, run_enc_case(key))
    for key, y in recorded:
        assert np.isfinite(y).all(), f"{key}: the reference's output is not finite"
    fin = {w: orig_steps_decode_finite(w) for w in ("v", "eps")}
    print(f"decode(use_original_steps=True) finite in the reference: {fin}")
    out["orig_steps_decode_finite/v"], out["orig_steps_decode_finite/eps"] = np.bool_(fin["v"]), np.bool_(fin["eps"])
    out["orig_steps_decode_finite"] = np.bool_(fin["v"] or fin["eps"])
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
