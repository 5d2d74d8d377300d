"""GPU: the img2img path on the kernels - pm_q_sample (bit-exact against the three-operation f32 expression), the sampler's
stochastic_encode / decode / `timesteps=` subset on HipOps against tests/golden/ddim_small_partial.npz (the REAL reference's
sampler at base width 64, tools/make_ddim_partial_golden.py), graph reuse between `sample` and `decode`, and the runner's
image_guided_refinement against its hand-written composition.

Trajectory bound: TRAJ_TOL_REDUCED of tests/test_unet_gpu.py (reduced-width forward floor x the cfg-4 guidance amplification:
5.6e-3 f16 / 4.4e-2 bf16) - every case here is a cfg-4 trajectory that is a SUFFIX of one that file already bounds that way.
Measured (printed as [parity] lines): see the docstring of test_partial_trajectories_on_the_kernels."""
import numpy as np
import pytest
import torch

from oracle import golden_recipe as gr
from open_pandora_amd import capi, synth, wm
from open_pandora_amd.autoencoder import DDCONFIG, AutoencoderKL
from open_pandora_amd.ddim import DDIMSampler
from test_ddim_partial_cpu import DECODE_CASES, ENC_CASES, SHAPE, golden, hand_composition, product_model, run_decode_case
from test_oracle_golden import rel
from test_unet_gpu import TRAJ_TOL_REDUCED

pytestmark = pytest.mark.gpu

NTAB = 10
GRID_CAP_THREADS = 2048 * 256  # pm_q_sample launches at most 2048 blocks of 256 threads: one pass of the grid-stride loop
PAD = 8                        # guard floats on either side of every operand (a multiple of 4: the aligned view stays aligned)
Q_SHAPES = [(1, 1), (1, 3), (1, 4), (3, 4 * 16 * 8 * 8 + 3), (2, 2048 * 256 * 4 + 5),  # the last: scalar path, several passes
            (2, 2048 * 256 * 2 + 4)]                                                     # 16-byte path, one item more than a pass
assert Q_SHAPES[-2][0] * Q_SHAPES[-2][1] > GRID_CAP_THREADS and Q_SHAPES[-1][0] * Q_SHAPES[-1][1] // 4 > GRID_CAP_THREADS
# which operands sit one float off the 16-byte grid (scalar path), and whether out is x0
Q_LAYOUTS = [("aligned", (0, 0, 0), False), ("x0_off", (1, 0, 0), False), ("noise_off", (0, 1, 0), False),
             ("out_off", (0, 0, 1), False), ("all_off", (1, 1, 1), False), ("in_place", (0, 0, 0), True),
             ("in_place_off", (1, 0, 1), True)]


def _guarded(values, off):
    """A NaN-filled buffer with `values` (B, n) at float offset PAD + off -> (buffer, the dense (B, n) view)."""
    B, n = values.shape
    buf = torch.full((B * n + 2 * PAD + 1,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[PAD + off:PAD + off + B * n].view(B, n)
    view.copy_(values)
    assert view.data_ptr() % 16 == (4 * off) % 16
    return buf, view


def _guards_intact(buf, off, count):
    return bool(torch.isnan(buf[:PAD + off]).all()) and bool(torch.isnan(buf[PAD + off + count:]).all())


@pytest.mark.parametrize("B,n", Q_SHAPES, ids=[f"{b}x{n}" for b, n in Q_SHAPES])
def test_q_sample_bit_exact(hip_ops_factory, B, n):
    """pm_q_sample against `a.view(B, 1) * x0 + s.view(B, 1) * noise` computed by torch in f32 on the host (two rounded products,
    one rounded sum - an FMA in the kernel would differ in the last bit of a good part of 10^4..10^6 elements): every layout of
    Q_LAYOUTS, table indices including 0 and NTAB - 1, NaN guards around every operand untouched."""
    ops = hip_ops_factory(torch.float16)
    g = torch.Generator().manual_seed(1000 + n)
    x0, noise = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    tab_a, tab_b = torch.rand(NTAB, generator=g) + 0.01, torch.rand(NTAB, generator=g) + 0.01
    for t in ([0, NTAB - 1, 4][:B] if B > 1 else [0], [NTAB - 1] * B):
        t = torch.tensor(t)
        want = tab_a[t].view(B, 1) * x0 + tab_b[t].view(B, 1) * noise
        for name, (ox, on, oo), in_place in Q_LAYOUTS:
            xb, xv = _guarded(x0, ox)
            nb, nv = _guarded(noise, on)
            ob, ov = (xb, xv) if in_place else _guarded(torch.full((B, n), float("nan")), oo)
            got = ops.q_sample(xv, nv, t, tab_a.cuda(), tab_b.cuda(), out=ov)
            assert got.data_ptr() == ov.data_ptr()
            assert torch.equal(got.cpu(), want), (name, t.tolist())
            assert _guards_intact(ob, ox if in_place else oo, B * n) and _guards_intact(nb, on, B * n), name
            assert torch.equal(nv.cpu(), noise) and (in_place or torch.equal(xv.cpu(), x0)), name
    # 5-D clips, no `out`: a fresh tensor, the inputs untouched; a host-side or a device-side index tensor
    if n == 4 * 16 * 8 * 8 + 3:
        x5, n5 = x0[:, :4096].reshape(B, 4, 16, 8, 8).cuda(), noise[:, :4096].reshape(B, 4, 16, 8, 8).cuda()
        t = torch.tensor([3, 0, 9])
        want = (tab_a[t].view(B, 1) * x0[:, :4096] + tab_b[t].view(B, 1) * noise[:, :4096]).reshape(x5.shape)
        for tt in (t, t.cuda()):
            assert torch.equal(ops.q_sample(x5, n5, tt, tab_a.cuda(), tab_b.cuda()).cpu(), want)


def test_q_sample_argument_checks(hip_ops_factory):
    """NULL operands -> PM_E_NULL, bad shapes -> PM_E_SHAPE (argument checks only: nothing is launched); an index outside the
    tables is the wrapper's ValueError, before any launch."""
    ops = hip_ops_factory(torch.float16)
    lib = capi.load()
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    p, tp, st = buf.data_ptr(), t.data_ptr(), ops._stream()
    good = [p, p, tp, p, p, p]
    for i in range(6):
        args = list(good)
        args[i] = 0
        assert lib.pm_q_sample(*args, 1, 4, 10, st) == -3  # PM_E_NULL
    for B, n, ntab in ((0, 4, 10), (1, 0, 10), (1, 4, 0), (-1, 4, 10)):
        assert lib.pm_q_sample(*good, B, n, ntab, st) == -2  # PM_E_SHAPE
    x = torch.ones(2, 8, device="cuda")
    tab = torch.ones(NTAB, device="cuda")
    for bad in ([0, NTAB], [-1, 0]):
        with pytest.raises(ValueError, match="indices"):
            ops.q_sample(x, x, torch.tensor(bad), tab, tab)
        with pytest.raises(ValueError, match="indices"):
            ops.q_sample(x, x, torch.tensor(bad).cuda(), tab, tab)
    torch.cuda.synchronize()
    assert bool((x == 1).all())


@pytest.mark.parametrize("key", list(ENC_CASES))
def test_stochastic_encode_on_the_kernel_bit_equal(hip_ops_factory, key):
    g = golden()
    smp = DDIMSampler(product_model("v", hip_ops_factory(torch.float16)))
    smp.make_schedule(10, "uniform_trailing", 0.0, verbose=False)
    out = smp.stochastic_encode(torch.from_numpy(g[f"{key}/x0"]).cuda(), torch.from_numpy(g[f"{key}/t"]),
                                use_original_steps=ENC_CASES[key], noise=torch.from_numpy(g[f"{key}/noise"]))
    assert out.is_cuda and out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), g[f"{key}/out"])
    with pytest.raises(ValueError, match="indices"):
        smp.stochastic_encode(out, torch.tensor([1000 if ENC_CASES[key] else 10] * out.shape[0]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("key", list(DECODE_CASES) + ["v_S10_subset6"])
def test_partial_trajectories_on_the_kernels(hip_ops_factory, dtype, key):
    """stochastic_encode -> decode (and the `timesteps=6` subset) on HipOps with the recipe's step noises against the real
    reference's f32 result.  Bound: TRAJ_TOL_REDUCED[dtype] (module docstring).  Measured f16 / bf16: v_S10_eta0_cfg4_t6
    2.55e-3 / 2.04e-2, v_S20_eta1_cfg4_t12 3.12e-3 / 2.31e-2, eps_S10_eta0_cfg4_t6 1.79e-3 / 1.33e-2, v_S10_subset6
    1.94e-3 / 1.72e-2."""
    g = golden()
    which = "v" if key == "v_S10_subset6" else DECODE_CASES[key][0]
    pm = product_model(which, hip_ops_factory(dtype))
    if key == "v_S10_subset6":
        ins, cond, uc = gr.sampler_inputs(8, 8)
        dev = lambda c: {k: [v.cuda() for v in lst] for k, lst in c.items()}
        smp = DDIMSampler(pm)
        smp.make_schedule(10, "uniform_trailing", 0.0, verbose=False)
        y, _ = smp.ddim_sampling(dev(cond), SHAPE, x_T=ins["x_T"].cuda(), timesteps=6, unconditional_guidance_scale=4.0,
                                 unconditional_conditioning=dev(uc), verbose=False,
                                 fs=torch.tensor([int(g["subset_fs"])]).cuda())
    else:
        z, y, _ = run_decode_case(pm, key, dev=lambda t: t.cuda(), spy=False)
        assert np.array_equal(z.cpu().numpy(), g[f"{key}/z"])
    err = rel(y.cpu(), g[f"{key}/out"])
    print(f"\n[parity] ddim partial {key} {dtype}: rel err {err:.2e}")
    assert y.dtype == torch.float32 and err <= TRAJ_TOL_REDUCED[dtype]


def test_decode_after_sample_replays_the_live_graph(hip_ops_factory):
    """sample(S = 10) captures the CFG forwards once; a decode on the SAME condition tensors replays that graph (no second
    capture) and gives what the eager decode gives, bit for bit."""
    g = golden()
    key = "v_S10_eta0_cfg4_t6"
    pm = product_model("v", hip_ops_factory(torch.float16))
    ins, cond, uc = gr.sampler_inputs(8, 8)
    dev = lambda c: {k: [v.cuda() for v in lst] for k, lst in c.items()}
    cond, uc, fs = dev(cond), dev(uc), torch.tensor([15]).cuda()
    smp = DDIMSampler(pm, use_graph=True)
    smp.sample(S=10, batch_size=1, shape=SHAPE[1:], conditioning=cond, verbose=False, unconditional_guidance_scale=4.0,
               unconditional_conditioning=uc, eta=0.0, fs=fs, timestep_spacing="uniform_trailing", x_T=ins["x_T"].cuda())
    assert len(smp._graphs) == 1
    live = next(iter(smp._graphs.values()))
    z = smp.stochastic_encode(torch.from_numpy(g[f"{key}/x0"]), torch.tensor([5]), noise=torch.from_numpy(g[f"{key}/enc_noise"]))
    y = smp.decode(z, cond, 6, 4.0, uc, fs=fs, verbose=False)
    assert len(smp._graphs) == 1 and next(iter(smp._graphs.values())) is live
    eager = DDIMSampler(pm, use_graph=False)
    eager.make_schedule(10, "uniform_trailing", 0.0, verbose=False)
    y2 = eager.decode(z, cond, 6, 4.0, uc, fs=fs, verbose=False)
    assert not eager._graphs and torch.equal(y, y2) and bool(torch.isfinite(y).all())
    smp.close()


def test_runner_refinement_on_the_gpu(hip_ops_factory):
    """wm.DiffusionRunner.image_guided_refinement at reduced width (U-Net 64 base channels, first stage ch 32, as
    tests/test_frames_gpu.py) from a latent and from 16 frames of 64 x 64: finite frames, equal to the hand-written
    composition bit for bit, the first stage called with at most 4 frames."""
    ops = hip_ops_factory(torch.float16)
    pm = product_model("v", ops)
    ae = AutoencoderKL(ddconfig=dict(DDCONFIG, ch=32))
    ae.load_state_dict(synth.synth_state_dict(ae, seed=gr.WEIGHT_SEED))
    ae.bind(ops)
    ins, _, _ = gr.sampler_inputs(8, 8)
    text, img = ins["c_crossattn"][:, :77].cuda(), ins["c_crossattn"][:, 77:].cuda()
    uct, uci = ins["uc_crossattn"][:, :77].cuda(), ins["uc_crossattn"][:, 77:].cuda()
    seen = []

    def encode(x, noise=None):
        seen.append(x.shape[0])
        return ae.encode_first_stage(x, noise=torch.zeros(x.shape[0], 4, x.shape[2] // 8, x.shape[3] // 8))

    run = wm.DiffusionRunner(pm, lambda im: img if float(im.abs().sum()) > 0 else uci, uct, encode, ae.decode_first_stage)
    frame0 = gr.ae_pixels(1, 64, 64).permute(1, 0, 2, 3)[None].cuda()          # (1, 3, 1, 64, 64)
    frames = gr.ae_pixels(16, 64, 64).permute(1, 0, 2, 3)[None].cuda()         # (1, 3, 16, 64, 64)
    enc_noise, ns = torch.from_numpy(golden()["enc_t0/noise"]), gr.noises(SHAPE, 2)
    kw = dict(ddim_steps=20, ddim_eta=1.0, unconditional_guidance_scale=4.0, fs=15, timestep_spacing="uniform_trailing")
    flat = frames[0].permute(1, 0, 2, 3)
    z_frames = torch.cat([encode(flat[i:i + 4]) for i in range(0, 16, 4)], 0).permute(1, 0, 2, 3)[None]
    for init, z_init, calls in ((gr.ae_latent(16, 8, 8).cuda(), gr.ae_latent(16, 8, 8).cuda(), [1]),
                                (frames, z_frames, [1, 4, 4, 4, 4])):
        del seen[:]
        got = run.image_guided_refinement(text, frame0, frame0[:, :, 0], init, 0.1, encode_noise=enc_noise,
                                          noise_fn=lambda i, shape: ns[i], **kw)
        assert seen == calls
        want = hand_composition(run, text, frame0, frame0[:, :, 0], z_init, 2, 20, 1.0, 4.0, 15, "uniform_trailing",
                                enc_noise, ns)
        want = ae.decode_first_stage(want)
        assert got.shape == (1, 1, 3, 16, 64, 64) and bool(torch.isfinite(got).all())
        assert torch.equal(got[:, 0], want)
    run.sampler.close()
