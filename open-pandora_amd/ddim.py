"""DDIMSampler: the S-step denoising loop of the hot path (drop-in for
lvdm.models.samplers.ddim.DDIMSampler, ddim.py:10-290).

Same call surface: `DDIMSampler(model).sample(S, batch_size, shape, conditioning, ..., eta, x_T,
unconditional_guidance_scale, unconditional_conditioning, precision, fs, timestep_spacing,
guidance_rescale, **kwargs)` -> (samples, intermediates), including the gradio progress kwargs
(`gr_progress_bar`, `round_info`, ddim.py:171-176).  Differences underneath:

* the latent stays f32 on the device for the whole loop; per step the two U-Net outputs, the CFG
  combine, v->eps / v->x0, dynamic rescale and the x_{t-1} update are ONE fused kernel
  (pm_ddim_update) instead of ~10 elementwise launches (ddim.py:238-288);
* all per-step scalars are computed once on the host with the reference's exact arithmetic
  (bf16-quantised tables, f64 sigmas cast to f32, f32 `1 - a_prev - sigma^2`), so the reference's
  numerics quirks are reproduced, including the NaN of S=10 / eta=1 / 'uniform_trailing' (SURVEY §0.5);
* `stochastic_encode` / `decode` (ddim.py:292-328), the img2img pair that starts from a given latent instead of pure noise, and
  the `timesteps=` subset of `ddim_sampling` run on the same step: the noising is one kernel (pm_q_sample), the partial loop is
  p_sample_ddim.  The original-step (1000-step) variants of the loops raise: the reference's own result is non-finite there;
* noise comes from an injectable `noise_fn(step_index, shape) -> f32 tensor` (default: torch.randn
  on the device), so both sides of a parity run can consume the same draws.
"""
import os

import numpy as np
import torch

_CAPTURE_STREAMS = {}

# decode(use_original_steps=True) / ddim_sampling(ddim_use_original_steps=True), ddim.py:252-256,296
_ORIGINAL_STEPS = ("the 1000-step (original DDPM steps) trajectory is not built: the reference's own result is non-finite on this "
                   "fork's bf16 schedule buffers - alphas_cumprod[0] rounds to 1.0, so ddim_sigmas_for_original_num_steps[0] is "
                   "0 / 0 (ddim.py:60-62) and every such trajectory ends at index 0; with use_dynamic_rescale it also reads "
                   "ddim_scale_arr[index], a table of S entries - there is nothing finite to compare against.  "
                   "stochastic_encode(use_original_steps=True) is finite in the reference and is available")


def _capture_streams(dev):
    """ONE long-lived (capture, second-branch) stream pair per device.  HipOps keeps a split-K workspace (256 MB) and
    the fp8 pack buffers per raw stream handle: a fresh pair per captured graph - a re-capture happens whenever the
    condition tensors move, e.g. every round of generate_multiround - pinned another set each time, and a capture
    on torch's own default capture stream never saw the workspace warmed up for it."""
    key = torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device()
    if key not in _CAPTURE_STREAMS:
        _CAPTURE_STREAMS[key] = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
    return _CAPTURE_STREAMS[key]


def _sqrt_f32(x):
    """The correctly rounded f32 square root of every entry of an f32 host tensor - what torch.sqrt / np.sqrt of that tensor
    give on a host whose vector square root is IEEE-exact, and what the reference's fixtures therefore hold.  Not torch.sqrt
    itself: its vectorised CPU kernel was measured one ulp off on one host (sqrt(0x1.c6p-1) = 0x1.e220eep-1 for the exact
    0x1.e220ecp-1, 4 of the 10 entries of an S = 10 table), and stochastic_encode is held to bit equality.  The scalar f64
    square root of the C library is exact everywhere, and rounding it to f32 is the exact f32 result (a 53-bit square root
    rounded to 24 bits cannot double-round: 53 >= 2 x 24 + 2)."""
    import math
    return torch.tensor([math.sqrt(v) for v in x.to(torch.float64).tolist()], dtype=torch.float64).to(torch.float32)


def make_ddim_timesteps(method, num_ddim, num_ddpm):
    """utils_diffusion.py:56-76."""
    if method == "uniform":
        c = num_ddpm // num_ddim
        return np.asarray(list(range(0, num_ddpm, c))) + 1
    if method == "uniform_trailing":
        c = num_ddpm / num_ddim
        return np.flip(np.round(np.arange(num_ddpm, 0, -c))).astype(np.int64) - 1
    if method == "quad":
        return ((np.linspace(0, np.sqrt(num_ddpm * 0.8), num_ddim)) ** 2).astype(int) + 1
    raise NotImplementedError(f'There is no ddim discretization method called "{method}"')


def _per_frame_kwargs(kwargs):
    """Does a pass-through kwarg carry tensors sized for ONE clip (features_adapter: (T, C, H, W) per level)?"""
    return any(torch.is_tensor(v) or (isinstance(v, (list, tuple)) and any(torch.is_tensor(w) for w in v)) for v in kwargs.values())


def _cfg_batchable(ops, x, c, uc, kwargs, extra=()):
    """PANDORA_CFG_BATCH=1 applies: ONE gate for the graph path and the eager path (the graph path skipped the
    op table's capability check, and neither looked at kwargs - a features_adapter sized for T frames met a forward over 2 T
    frames and failed the shape assert inside the capture).  Per-clip tensors in kwargs -> the two-forward form."""
    return (uc is not None and not extra and os.environ.get("PANDORA_CFG_BATCH", "0") == "1" and isinstance(c, dict)
            and isinstance(uc, dict) and set(c) == set(uc) and x.shape[0] == 1
            and getattr(ops, "supports_batched_clips", True) and not _per_frame_kwargs(kwargs))


def _version_of(v):
    """In-place-edit counter for the graph keys; tensors created under torch.inference_mode() track none (reading
    `_version` raises there) and cannot be edited in place outside it either: 0."""
    return 0 if v.is_inference() else v._version


class _ForwardGraph:
    """The U-Net forwards of one DDIM step (cond and, with CFG, uncond) captured once into a HIP graph
    and replayed every step: ~2000 kernel launches per step become one graph launch.  Inputs live in
    static buffers (latent, timestep); the condition tensors are read in place at replay.

    The two forwards of a CFG step are independent (ddim.py:233-234 runs them back to back): they are captured
    on TWO streams forked inside the graph, so their kernels overlap on the device - the forward is a chain of
    ~1100 dependent launches averaging 25 us, half of them on grids that do not fill 256 CUs (the 10x16 and 5x8
    levels) and each with a ramp and a tail; a second, independent chain fills those holes.
    (PANDORA_CFG_STREAMS=0: one stream, the two forwards in sequence.)"""

    def __init__(self, model, x, t, c, uc, fs, kwargs, extra=(), ops=None):
        """`extra`: further condition sets whose forwards join the graph (the multi-condition sampler's third,
        image-only branch, ddim_multiplecond.py:232): captured on the main stream behind the conditional forward."""
        self.x = x.clone()
        self.t = t.clone()
        self.cc = None
        dev = x.device
        side, other = _capture_streams(dev)
        # PANDORA_CFG_BATCH=1: the cond / uncond pair as ONE forward over 2 x T frames (UNetModel batches the clips along the
        # rows: weights read once, grids twice as full) instead of two forwards on two streams
        self.batched = _cfg_batchable(ops, x, c, uc, kwargs, extra)
        if self.batched:
            # static copies of the stacked conditions: the graph reads THESE at every replay, so they live as long as it does
            # (kept on self: as locals they were freed at the end of __init__ and the next eager allocation overwrote them)
            cc = self.cc = {k: [torch.cat([a, b_], 0) for a, b_ in zip(c[k], uc[k])] for k in c}
            self.x = torch.cat([x, x], 0)
            self.t = torch.cat([t, t], 0)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):  # warm-up outside capture
                model.apply_model(self.x, self.t, cc, fs=fs, **kwargs)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
                out = model.apply_model(self.x, self.t, cc, fs=fs, **kwargs)
            self.e_c, self.e_u, self.e_x = out[0:1], out[1:2], []
            return
        two = uc is not None and os.environ.get("PANDORA_CFG_STREAMS", "1") != "0"
        if not two:
            other = None
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm-up outside capture: packs weights, sizes the allocator
            model.apply_model(self.x, self.t, c, fs=fs, **kwargs)
        torch.cuda.current_stream(dev).wait_stream(side)
        if two:  # and the second stream's split-K workspace (HipOps keeps one per stream)
            other.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(other):
                model.apply_model(self.x, self.t, uc, fs=fs, **kwargs)
            torch.cuda.current_stream(dev).wait_stream(other)
            torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        # thread-local capture mode: under the default (global) mode a HIP call made by ANY other thread of the process
        # while this capture is open fails AND invalidates the capture - e.g. the event query of a torch.distributed
        # watchdog thread that is still polling the last collective of a previous (sharded) run, which then takes the
        # process down from that thread (the r03 abort of tests/test_segmented_gpu.py), or another
        # gradio worker's allocation.  This capture only needs ITS thread's calls to be capturable.
        with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):  # (the stream whose workspace the warm-up sized)
            main = torch.cuda.current_stream(dev)
            if two:
                other.wait_stream(main)  # fork
                with torch.cuda.stream(other):
                    self.e_u = model.apply_model(self.x, self.t, uc, fs=fs, **kwargs)
            self.e_c = model.apply_model(self.x, self.t, c, fs=fs, **kwargs)
            self.e_x = [model.apply_model(self.x, self.t, cx, fs=fs, **kwargs) for cx in extra]
            if two:
                main.wait_stream(other)  # join
            else:
                self.e_u = model.apply_model(self.x, self.t, uc, fs=fs, **kwargs) if uc is not None else None

    def __call__(self, x, t):
        if self.batched:
            self.x[0:1].copy_(x)
            self.x[1:2].copy_(x)
            self.t.copy_(t.expand(2))
        else:
            self.x.copy_(x)
            self.t.copy_(t)
        self.graph.replay()
        return self.e_c, self.e_u

    def close(self):
        """Drop the graph and the outputs that live in its private pool (DDIMSampler.close)."""
        self.graph = self.e_c = self.e_u = self.cc = None
        self.e_x = []


class _SegmentedForward:
    """A frame-sharded U-Net forward (frame_parallel.FrameParallel) has ~140 exchanges inside, which a HIP graph of
    the whole forward cannot hold; issued eagerly, its ~1100 launches cost ~10 ms of host time per forward - more
    than the sharded kernels take at 4 or 8 ranks.  Here the kernels BETWEEN two exchanges are captured as HIP
    graphs that share one memory pool, and a step replays [graph 0, exchange 0, graph 1, ..., graph n] in order:
    the exchanges stay ordinary RCCL calls on the replay stream, re-issued on the buffers they were recorded
    with (FrameParallel allocates them before the call, inside the preceding segment, from the graphs' pool).
    Recording executes each segment right after capturing it (graph replay), so every exchange sees real data and
    all ranks walk the same sequence of collectives as an eager forward."""

    def __init__(self, model, x, t, c, fs, kwargs, fp):
        self.x, self.t = x.clone(), t.clone()
        dev = x.device
        self._side = _capture_streams(dev)[0]
        self._side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self._side):  # warm-up on the capture stream: weights packed, split-K scratch sized
            model.apply_model(self.x, self.t, c, fs=fs, **kwargs)
        torch.cuda.current_stream(dev).wait_stream(self._side)
        torch.cuda.synchronize(dev)
        self.steps = []
        self._pool = torch.cuda.graph_pool_handle()
        self._ctx = None
        fp.recorder = self
        try:
            self._begin()
            self.out = model.apply_model(self.x, self.t, c, fs=fs, **kwargs)
            self._end()
        except BaseException:
            if self._ctx is not None:  # leave capture mode before the caller falls back to an eager forward
                try:
                    self._ctx.__exit__(None, None, None)
                except Exception:
                    pass
            raise
        finally:
            fp.recorder = None

    def _begin(self):
        self._g = torch.cuda.CUDAGraph()
        # thread-local capture mode: the process group's watchdog thread polls events of the exchanges just issued while
        # the next segment is being captured; under the default (global) mode its calls would invalidate the capture
        self._ctx = torch.cuda.graph(self._g, pool=self._pool, stream=self._side, capture_error_mode="thread_local")
        self._ctx.__enter__()

    def _end(self):
        self._ctx.__exit__(None, None, None)
        self._ctx = None
        self.steps.append(self._g)

    def comm(self, fn):
        self._end()
        self._g.replay()  # run the segment just captured: the exchange needs its real outputs
        fn()
        self.steps.append(fn)
        self._begin()

    def __call__(self, x, t):
        self.x.copy_(x)
        self.t.copy_(t)
        for s in self.steps:
            if isinstance(s, torch.cuda.CUDAGraph):
                s.replay()
            else:
                s()
        return self.out

    def close(self):
        """Drop the segment graphs, the recorded exchange closures (they hold the exchange buffers, which live in the
        graphs' pool) and the pool handle - in that order, after the device has drained (DDIMSampler.close)."""
        self.steps = []
        self.out = self._g = self._pool = None


def _segments_supported(fp, dev):
    """Collective go / no-go for the segmented replay (a per-rank fallback leaves the ranks at different
    points of the exchange sequence).  Every rank of the frame group runs the same tiny rehearsal - capture, RCCL call
    next to the capture, capture - and the minimum of the outcomes decides for ALL of them.  The sequence of collectives
    is the same on every path: a rank whose capture raised still issues the rehearsal all-reduce (on a
    plain buffer) before the flag exchange, so RCCL never pairs collectives of different size / dtype."""
    import torch.distributed as dist
    from .frame_parallel import control_collective
    ok = 1
    side = _capture_streams(dev)[0]
    buf = pool = None

    def segment():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=pool, stream=side, capture_error_mode="thread_local"):
            buf.add_(1.0)
        g.replay()

    try:
        side.wait_stream(torch.cuda.current_stream(dev))
        pool = torch.cuda.graph_pool_handle()
        with torch.cuda.stream(side):
            buf = torch.zeros(64, device=dev)
        segment()
    except Exception:  # noqa: BLE001 - any failure means "eager", decided below for every rank at once
        ok = 0
    try:
        if buf is None:
            buf = torch.zeros(64, device=dev)
        with torch.cuda.stream(side):
            rec, fp.recorder = fp.recorder, None
            try:  # (through FrameParallel._comm: RCCL calls never run on a stream that captures, see there)
                fp._comm(lambda: dist.all_reduce(buf, group=fp.group))
            finally:
                fp.recorder = rec
    except Exception:  # noqa: BLE001
        ok = 0
    try:
        if ok:
            segment()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
    except Exception:  # noqa: BLE001
        ok = 0
    flag = torch.tensor([ok], device=dev if fp.backend == "nccl" else "cpu", dtype=torch.int32)
    control_collective(lambda: dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=fp.group), fp.group)
    return bool(flag.item())


class DDIMSampler:
    multicond = False  # DDIMSamplerMultiCond: three forwards per step (text + image guidance, ddim_multiplecond.py:214-234)

    def __init__(self, model, schedule="linear", use_graph=None, cfg_parallel=None, ops=None, **kwargs):
        """`ops`: the op table for the fused update kernel; default = the one bound to model's U-Net.  Pass it
        explicitly to run this sampler around a model whose U-Net is not ours (e.g. the reference's own
        LatentVisualDiffusion shell: the sampler only needs the attributes of ddim.py:14,27-50,229-277)."""
        self.model = model
        self._ops_override = ops
        self.cfg_parallel = cfg_parallel  # frame_parallel.CFGParallel: this rank runs ONE CFG branch
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.counter = 0
        # HIP-graph replay of the forwards (single-GPU HipOps only; PANDORA_HIPGRAPH=0 disables)
        self.use_graph = (os.environ.get("PANDORA_HIPGRAPH", "1") != "0") if use_graph is None else use_graph
        self._graphs = {}
        self._seg_failed = False  # the frame group decided against segmented replay (or, at one rank, a capture raised)
        self._seg_probed = False
        self._gen = None  # multi-rank noise generator (see _draw)
        self._enc_tables = {}  # stochastic_encode's device tables (see make_schedule)

    def close(self, twin=True):
        """Release every captured graph of this sampler: the device drains, the graphs, the exchange closures recorded
        between them and their private memory pools go, the device drains again.  Call it before
        `dist.destroy_process_group()` (and before dropping the op table): the recorded exchanges hold RCCL-registered
        buffers and the pools hold the activations of a forward (explicit lifetimes instead of whatever
        order the garbage collector picks at interpreter exit)."""
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        for g in self._graphs.values():
            g.close()
        self._graphs.clear()
        other = getattr(self, "_multicond_twin", None)  # wm._multicond_sampler: the cached multi-condition sampler
        if twin and other is not None:
            other.close()
        import gc
        gc.collect()
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()

    def _fp(self):
        unet = getattr(getattr(self.model, "model", None), "diffusion_model", None)
        return getattr(unet, "fp", None)

    def _multi_rank(self):
        return self.cfg_parallel is not None or self._fp() is not None

    def _draw(self, shape, device):
        """Standard-normal draw of CLIP-level shape.  Single process: the device RNG, as the reference
        (lvdm/common.py:31-34).  Multi-rank (CFG pair and / or frame shards): every rank must consume the SAME
        clip-level draw - the partners of a CFG pair apply the identical update, a frame shard takes its slice of
        one clip - so all ranks draw the full tensor from a generator seeded with a value broadcast by rank 0."""
        if not self._multi_rank():
            return torch.randn(shape, device=device)
        if self._gen is None:
            import torch.distributed as dist
            seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)
            t = seed.to(device) if dist.get_backend() == "nccl" else seed
            from .frame_parallel import control_collective
            control_collective(lambda: dist.broadcast(t, src=0))
            # a generator ON the device: identical GPUs give identical Philox streams, and no host randn + blocking
            # H2D copy sits in the step loop
            self._gen = torch.Generator(device=device).manual_seed(int(t.item()))
        return torch.randn(shape, generator=self._gen, device=device)

    def _ops(self):
        ops = self._ops_override or getattr(self.model, "ops", None)
        if ops is None:
            ops = getattr(self.model.model.diffusion_model, "ops", None)
        if ops is None:
            raise RuntimeError("the U-Net has no op table bound (UNetModel.bind(HipOps(...)))")
        return ops

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        """Per-step scalar tables (ddim.py:24-63 + utils_diffusion.py:79-91), kept on the host."""
        m = self.model
        ts = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps)
        self.ddim_timesteps = ts
        ac32 = m.alphas_cumprod.detach().to(torch.float32).cpu()  # bf16-quantised values, as f32
        assert ac32.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        idx = torch.as_tensor(np.ascontiguousarray(ts), dtype=torch.long)
        a32 = ac32[idx]
        a = a32.to(torch.float64)
        a_prev = torch.cat([ac32[0:1], ac32[idx[:-1]]]).to(torch.float64)
        # reference arithmetic (utils_diffusion.py:86): `alphas` is an f32 tensor and `alphas_prev` a
        # float64 ndarray, so `(1 - alphas_prev) / (1 - alphas)` runs as ndarray.__truediv__ ->
        # Tensor.__rtruediv__ = f32 reciprocal(1 - alphas) * float64 array; the rest is float64.
        sig = (1 - a32).reciprocal().to(torch.float64) * (1 - a_prev) * (1 - a / a_prev)
        sig = torch.from_numpy(ddim_eta * np.sqrt(sig.numpy()))  # np.sqrt as in the reference
        self.ddim_alphas = a32
        self.ddim_alphas_prev = a_prev.numpy()
        self.ddim_sigmas = sig
        self.ddim_sqrt_one_minus_alphas = torch.sqrt(1.0 - self.ddim_alphas)
        if m.use_dynamic_rescale:
            sa = m.scale_arr.detach().cpu()[idx]
            self.ddim_scale_arr = sa
            self.ddim_scale_arr_prev = torch.cat([sa[0:1], sa[:-1]])
        self._sqrt_ac = m.sqrt_alphas_cumprod.detach().to(torch.float32).cpu().numpy()
        self._sqrt_1mac = m.sqrt_one_minus_alphas_cumprod.detach().to(torch.float32).cpu().numpy()
        self._enc_tables = {}  # stochastic_encode's device tables: formed on first use, dropped with the schedule

    def step_scalars(self, index, step):
        """f32 scalars of p_sample_ddim (ddim.py:252-288) for the fused update kernel: v- and eps-parameterisation."""
        f32 = np.float32
        a_prev = f32(self.ddim_alphas_prev[index])
        sigma = f32(self.ddim_sigmas[index].item())
        with np.errstate(invalid="ignore"):
            dir_coef = np.sqrt(f32(f32(1.0) - a_prev) - f32(sigma * sigma), dtype=f32)
        rescale = f32(1.0)
        if self.model.use_dynamic_rescale:
            rescale = f32(self.ddim_scale_arr_prev[index].item()) / f32(self.ddim_scale_arr[index].item())
        if getattr(self.model, "parameterization", "v") == "eps":
            # eps-prediction (the 256 yaml's class default; ddim.py:245-246,265-266): e_t = model output,
            #     pred_x0 = (x - s1 e_t) / sa * r,    x_prev = P pred_x0 + D e_t + noise,    sa = sqrt(a_t), s1 = sqrt(1 - a_t).
            # The fused kernel computes  eps_k = A v + B x,  x0_k = (A x - B v) R,  x_prev = P' x0_k + D' eps_k  (pm_ddim_update).
            # With A = 1, B = s1, R = r / sa its x0_k IS pred_x0, and eps_k = v + s1 x = (1 + s1^2) v + (s1 sa / r) x0_k, so
            # D' = D / (1 + s1^2), P' = P - D' s1 sa / r give the reference's update exactly (f64 here, f32 in the kernel):
            # no second kernel flavour for a parameterisation Open-Pandora itself does not ship.
            sa = float(np.sqrt(f32(self.ddim_alphas[index].item()), dtype=f32))
            s1 = float(f32(self.ddim_sqrt_one_minus_alphas[index].item()))
            P, D, r = float(np.sqrt(a_prev, dtype=f32)), float(dir_coef), float(rescale)
            Dk = D / (1.0 + s1 * s1)
            return dict(sqrt_ac=1.0, sqrt_1mac=s1, rescale=r / sa, sqrt_a_prev=P - Dk * s1 * sa / r, dir_coef=Dk,
                        sigma=float(sigma))
        return dict(sqrt_ac=float(self._sqrt_ac[step]), sqrt_1mac=float(self._sqrt_1mac[step]),
                    rescale=float(rescale), sqrt_a_prev=float(np.sqrt(a_prev, dtype=f32)),
                    dir_coef=float(dir_coef), sigma=float(sigma))

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0,
               noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, verbose=True,
               schedule_verbose=False, x_T=None, log_every_t=100, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, precision=None, fs=None, timestep_spacing="uniform",
               guidance_rescale=0.0, **kwargs):
        if conditioning is not None and isinstance(conditioning, dict):
            first = conditioning[list(conditioning.keys())[0]]
            cbs = (first[0] if isinstance(first, (list, tuple)) else first).shape[0]
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        if quantize_x0:  # (ddim.py:277-278: first_stage_model.quantize - a VQ first stage; Open-Pandora ships the KL autoencoder)
            raise NotImplementedError("quantize_x0 needs a VQ first stage; the Open-Pandora first stage is AutoencoderKL")
        if score_corrector is not None and self._fp() is not None:
            raise NotImplementedError("score_corrector sees one rank's frames only in frame-sharded mode")
        if noise_dropout > 0.0 and self._multi_rank():
            raise NotImplementedError("noise_dropout draws its mask from this rank's RNG: the ranks of one clip would diverge")
        self.make_schedule(ddim_num_steps=S, ddim_discretize=timestep_spacing, ddim_eta=eta, verbose=schedule_verbose)
        size = (batch_size, *shape)
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback, mask=mask,
                                  x0=x0, temperature=temperature, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, verbose=verbose,
                                  precision=precision, fs=fs, guidance_rescale=guidance_rescale,
                                  noise_dropout=noise_dropout, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, **kwargs)

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, temperature=1.0, unconditional_guidance_scale=1.0,
                      unconditional_conditioning=None, fs=None, noise=None, want_x0=True, step=None,
                      guidance_rescale=0.0, cfg_img=None, unconditional_conditioning_img_nonetext=None,
                      noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, **kwargs):
        """One denoising step (ddim.py:218-290): two U-Net forwards when CFG is on, then the fused
        update kernel.  `t` is the (b,) long tensor of the current DDPM timestep, `index` its position
        in the DDIM schedule.  `noise` (f32, x-shaped) overrides the device RNG draw."""
        ops = self._ops()
        if step is None:
            step = int(t[0])  # device sync; ddim_sampling passes the host-side value instead
        use_cfg = unconditional_conditioning is not None and unconditional_guidance_scale != 1.0
        uc = unconditional_conditioning if use_cfg else None
        unet = getattr(getattr(self.model, "model", None), "diffusion_model", None)
        graphable = (self.use_graph and getattr(ops, "supports_graphs", False) and isinstance(c, dict)
                     and getattr(unet, "fp", None) is None and x.is_cuda)
        pair = self.cfg_parallel is not None and use_cfg  # this rank runs ONE branch, then one exchange

        uc_img = unconditional_conditioning_img_nonetext if (self.multicond and use_cfg) else None
        if self.multicond and use_cfg:
            if uc_img is None:
                # (the reference calls apply_model(x, t, None) here and fails inside the U-Net, ddim_multiplecond.py:232;
                # model.py:737-743 only builds this condition set when cfg_img != 1.0)
                raise ValueError("the multi-condition sampler needs `unconditional_conditioning_img_nonetext` (image tokens + "
                                 "empty text, model.py:737-743) whenever unconditional_guidance_scale != 1")
            if self._multi_rank():
                raise NotImplementedError("the multi-condition sampler runs on one GPU (three forwards per step)")

        def replay(cc, uu, extra=()):
            if hasattr(unet, "packed") and getattr(unet, "ops", None) is not None:
                unet.packed()  # re-packs (and moves the pack epoch in the key below) after an in-place weight edit
            tensors = ([v for d in (cc, uu or {}) + tuple(extra) for lst in d.values() for v in lst]
                       + ([fs] if torch.is_tensor(fs) else []))
            for v in kwargs.values():  # tensors handed through to the U-Net (e.g. features_adapter): read in place by the graph
                tensors += [v] if torch.is_tensor(v) else [w for w in v if torch.is_tensor(w)] if isinstance(v, (list, tuple)) else []
            # (a weight reload / .to() re-packs the kernel-side weights: the captured graph holds raw pointers to the
            # old ones, so the U-Net's pack epoch is part of the key)
            key = (tuple(x.shape), tuple((v.data_ptr(), tuple(v.shape), _version_of(v)) for v in tensors), tuple(sorted(kwargs)),
                   getattr(unet, "_pack_epoch", 0), os.environ.get("PANDORA_CFG_BATCH", "0"))
            g = self._graphs.get(key)
            if g is None:
                for old in self._graphs.values():
                    old.close()
                self._graphs.clear()  # one live graph: its private pool holds a forward's activations
                g = self._graphs[key] = _ForwardGraph(self.model, x, t, cc, uu, fs, kwargs, extra, ops=ops)
            return g(x, t) + tuple(g.e_x)

        fp_u = getattr(unet, "fp", None)
        # frame shards: HIP graphs of the segments between the in-forward exchanges (RCCL; PANDORA_SEGMENT_GRAPHS=0 or a
        # failed capture: the eager forward; =force: also on gloo, whose exchanges then wait for the stream themselves -
        # the multi-process rehearsal of the recorder on one GPU, tests/test_peer_gpu.py)
        segmentable = (self.use_graph and getattr(ops, "supports_graphs", False) and isinstance(c, dict) and x.is_cuda
                       and fp_u is not None and not self._seg_failed
                       and (fp_u.backend == "nccl" or os.environ.get("PANDORA_SEGMENT_GRAPHS") == "force")
                       and os.environ.get("PANDORA_SEGMENT_GRAPHS", "1") != "0")

        if segmentable and not self._seg_probed and fp_u.world > 1:
            self._seg_probed = True
            if not _segments_supported(fp_u, x.device):
                import warnings
                warnings.warn("segmented graph replay is not available on this RCCL build (rehearsal failed on at "
                              "least one rank of the frame group): every rank issues the forward eagerly")
                self._seg_failed = True
                segmentable = False

        def forward_sharded(cc, slot):
            if segmentable:
                tensors = [v for lst in cc.values() for v in lst] + ([fs] if torch.is_tensor(fs) else [])
                # (the segments hold the peer mailbox's addresses by value: its generation is part of the key, ADVICE r03;
                # read again after a recording, whose warm-up forward may have re-created the mailbox for a larger halo)
                mk = lambda: ("seg", slot, tuple(x.shape), tuple((v.data_ptr(), tuple(v.shape), _version_of(v)) for v in tensors),
                              tuple(sorted(kwargs)), getattr(unet, "_pack_epoch", 0),
                              getattr(getattr(fp_u, "mailbox", None), "generation", 0))
                key = mk()
                g = self._graphs.get(key)
                if g is None:
                    for k in [k for k in self._graphs if k[0] == "seg" and k[1] == slot]:
                        self._graphs.pop(k).close()
                    try:
                        g = _SegmentedForward(self.model, x, t, cc, fs, kwargs, fp_u)
                        self._graphs[mk()] = g
                    except Exception as exc:  # e.g. an RCCL build that refuses calls next to a capture
                        if fp_u.world > 1:
                            # peers are somewhere inside the recorded exchange sequence: restarting this rank's forward
                            # eagerly would pair its first exchange with their k-th (hang or silently wrong data)
                            raise RuntimeError("segmented graph capture of the frame-sharded forward failed on this rank "
                                               "after the frame group's rehearsal succeeded; aborting instead of "
                                               "falling back locally (PANDORA_SEGMENT_GRAPHS=0 selects the eager "
                                               "forward on every rank)") from exc
                        import warnings
                        warnings.warn(f"segmented graph capture of the frame-sharded forward failed ({exc!r}): eager")
                        self._seg_failed = True
                        return self.model.apply_model(x, t, cc, fs=fs, **kwargs)
                return g(x, t)
            return self.model.apply_model(x, t, cc, fs=fs, **kwargs)

        if pair:
            # this rank runs ONE branch; the exchange of the two branch outputs stays outside any graph.  Without
            # frame shards the branch forward has no collective inside and replays as one graph
            mine = c if self.cfg_parallel.branch == 0 else uc
            if fp_u is not None:
                e_mine = forward_sharded(mine, 0)
            else:
                e_mine = replay(mine, None)[0] if graphable else self.model.apply_model(x, t, mine, fs=fs, **kwargs)
            e_c, e_u = self.cfg_parallel.exchange(e_mine)
        elif uc_img is not None:  # multi-condition: conditional, unconditional and image-only ("" text) forwards
            if graphable:
                e_c, e_u, e_ui = replay(c, uc, (uc_img,))
            else:
                e_c, e_u, e_ui = (self.model.apply_model(x, t, cc, fs=fs, **kwargs) for cc in (c, uc, uc_img))
        elif graphable and self.cfg_parallel is None:
            e_c, e_u = replay(c, uc)[:2]
        elif fp_u is not None:
            e_c = forward_sharded(c, 0)
            e_u = forward_sharded(uc, 1) if use_cfg else None
        elif use_cfg and _cfg_batchable(ops, x, c, uc, kwargs):
            cc = {k: [torch.cat([a, b_], 0) for a, b_ in zip(c[k], uc[k])] for k in c}
            out = self.model.apply_model(torch.cat([x, x], 0), torch.cat([t, t], 0), cc, fs=fs, **kwargs)
            e_c, e_u = out[0:1], out[1:2]
        else:
            e_c = self.model.apply_model(x, t, c, fs=fs, **kwargs)
            e_u = self.model.apply_model(x, t, uc, fs=fs, **kwargs) if use_cfg else None
        cfg_scale = float(unconditional_guidance_scale)
        if uc_img is not None:
            # ddim_multiplecond.py:233-236: text guidance on top of image guidance, then (optionally) rescale_noise_cfg against
            # the conditional output; the fused update kernel takes the finished model output (e_u = None, cfg = 1)
            ci = cfg_scale if cfg_img is None else float(cfg_img)
            v = e_u + ci * (e_ui - e_u) + cfg_scale * (e_c - e_ui)
            if guidance_rescale > 0.0:
                dims = list(range(1, e_c.dim()))
                resc = v * (e_c.std(dim=dims, keepdim=True) / v.std(dim=dims, keepdim=True))
                v = guidance_rescale * resc + (1.0 - guidance_rescale) * v
            e_c, e_u, cfg_scale = v, None, 1.0
        elif use_cfg and guidance_rescale > 0.0:
            # rescale_noise_cfg (utils_diffusion.py:147-158, ddim.py:240-241): match the guided output's
            # per-sample std to the conditional one, blended by guidance_rescale.  A reduction over the
            # whole (655k-element) model output: plain torch on the f32 outputs, then the fused update
            # kernel takes the finished model output (e_u = None, cfg = 1)
            dims = list(range(1, e_c.dim()))
            v = e_u + cfg_scale * (e_c - e_u)
            fp = self._fp()
            if fp is None:
                ratio = e_c.std(dim=dims, keepdim=True) / v.std(dim=dims, keepdim=True)
            else:
                # frame shards: the reference takes the std over the WHOLE (C, T, H, W) sample - one all-reduce of
                # {sum, sum of squares} of both tensors and the element count, then the same unbiased estimator
                ec64, v64 = e_c.double(), v.double()
                part = torch.stack([ec64.sum(), (ec64 * ec64).sum(), v64.sum(), (v64 * v64).sum(),
                                    torch.tensor(float(e_c.numel()), dtype=torch.float64, device=e_c.device)])
                tot = fp.all_reduce_sum(part)
                n = tot[4]
                std = lambda s1, s2: ((s2 - s1 * s1 / n) / (n - 1)).clamp_min(0).sqrt()
                ratio = (std(tot[0], tot[1]) / std(tot[2], tot[3])).to(v.dtype)
            v = guidance_rescale * (v * ratio) + (1.0 - guidance_rescale) * v
            e_c, e_u, cfg_scale = v, None, 1.0
        if score_corrector is not None:
            # ddim.py:248-250: the finished model output (guided, rescaled) goes through the corrector's modify_score before the
            # update - eps parameterisation only, as the reference asserts; the fused update kernel then takes e_t as it is
            assert self.model.parameterization == "eps", 'not implemented'
            e_t = e_c if e_u is None else e_u + cfg_scale * (e_c - e_u)
            e_t = score_corrector.modify_score(self.model, e_t, x, t, c, **(corrector_kwargs or {}))
            e_c, e_u, cfg_scale = e_t.to(torch.float32), None, 1.0
        sc = self.step_scalars(index, step)
        if sc["sigma"] != 0.0:
            if noise is None:
                fp = self._fp()
                if fp is None:
                    noise = self._draw(x.shape, ops.device)
                else:  # this rank's frames of ONE clip-level draw
                    clip = tuple(x.shape[:2]) + (fp.total_frames,) + tuple(x.shape[3:])
                    noise = fp.shard_frames(self._draw(clip, ops.device))
            noise = noise.to(device=ops.device, dtype=torch.float32).contiguous()
            if noise_dropout > 0.0:  # ddim.py:283-284 drops elements of sigma * noise * temperature: the scalars commute with the mask
                noise = torch.nn.functional.dropout(noise, p=noise_dropout).contiguous()
            sc["sigma"] *= float(temperature)
        else:
            noise = None
        return ops.ddim_update(x, e_c.contiguous(), None if e_u is None else e_u.contiguous(), noise,
                               cfg_scale, want_x0=want_x0, **sc)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, callback=None, mask=None, x0=None, img_callback=None,
                      log_every_t=100, temperature=1.0, unconditional_guidance_scale=1.0,
                      unconditional_conditioning=None, verbose=True, precision=None, fs=None,
                      noise_fn=None, guidance_rescale=0.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None,
                      timesteps=None, ddim_use_original_steps=False, **kwargs):
        """`timesteps=k` (ddim.py:163-165): only the first `int(min(k / S, 1) * S) - 1` entries of the schedule are walked -
        the reference's off-by-one kept as it is (k = 6 of S = 10 runs 5 steps)."""
        if ddim_use_original_steps:
            raise NotImplementedError(_ORIGINAL_STEPS)
        ops = self._ops()
        device = ops.device
        img = self._draw(shape, device) if x_T is None else x_T.to(device)
        img = img.to(torch.float32).contiguous()  # the loop state stays f32 (see module docstring)
        fp = self._fp()
        if fp is not None:
            # frame-sharded U-Net: `shape`, x_T, the concat condition and the noise are CLIP-level here (as the
            # caller of the reference's sampler passes them); this rank keeps its frames, the final latent is
            # gathered.  c_crossattn stays whole (the U-Net slices the per-frame image tokens itself).
            T_total = fp.total_frames
            shard = lambda t: fp.shard_frames(t.to(device)) if torch.is_tensor(t) and t.dim() == 5 and t.shape[2] == T_total else t
            img = shard(img)

            def shard_cond(c):
                if not isinstance(c, dict) or "c_concat" not in c:
                    return c
                return dict(c, c_concat=[shard(t) for t in c["c_concat"]])

            cond, unconditional_conditioning = shard_cond(cond), shard_cond(unconditional_conditioning)
            if noise_fn is not None:
                user_noise = noise_fn
                noise_fn = lambda i, shp: shard(user_noise(i, shape))
        if timesteps is None:
            timesteps = self.ddim_timesteps
        else:
            subset_end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1
            timesteps = self.ddim_timesteps[:subset_end]
        total_steps = timesteps.shape[0]
        time_range = np.flip(timesteps)
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        if kwargs.get("gr_progress_bar") is not None:
            ri = kwargs.get("round_info", [1, 1])
            iterator = kwargs["gr_progress_bar"].tqdm(time_range, desc=f"DDIM Sampler (Round {ri[0]}/{ri[1]})", total=total_steps)
        elif verbose:
            from tqdm import tqdm
            iterator = tqdm(time_range, desc="DDIM Sampler", total=total_steps)
        else:
            iterator = time_range
        clean_cond = kwargs.pop("clean_cond", False)
        model_kwargs = {k: v for k, v in kwargs.items()
                        if k not in ("gr_progress_bar", "round_info", "cfg_img", "unconditional_conditioning_img_nonetext")}
        b = shape[0]
        for i, step in enumerate(iterator):
            index = total_steps - i - 1
            step = int(step)
            ts = torch.full((b,), step, device=device, dtype=torch.long)
            if mask is not None:  # blend with the (noised) original latent, ddim.py:186-192
                assert x0 is not None
                img_orig = x0 if clean_cond else self.model.q_sample(x0, ts.cpu()).to(device)
                img = (img_orig * mask + (1.0 - mask) * img).float().contiguous()
            noise = noise_fn(i, shape) if noise_fn is not None else None
            if self.multicond:  # (ddim_multiplecond.py:190-196: these two reach p_sample_ddim there)
                model_kwargs = dict(model_kwargs, cfg_img=kwargs.get("cfg_img"),
                                    unconditional_conditioning_img_nonetext=kwargs.get("unconditional_conditioning_img_nonetext"))
            img, pred_x0 = self.p_sample_ddim(img, cond, ts, index, temperature=temperature,
                                              unconditional_guidance_scale=unconditional_guidance_scale,
                                              unconditional_conditioning=unconditional_conditioning, fs=fs,
                                              noise=noise, step=step,
                                              guidance_rescale=guidance_rescale, noise_dropout=noise_dropout,
                                              score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
                                              **model_kwargs)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates["x_inter"].append(img)
                intermediates["pred_x0"].append(pred_x0)
        if fp is not None:
            img = fp.gather_frames(img)
            if getattr(fp, "mailbox", None) is not None:
                # once per clip, on every rank: a timed-out peer exchange invalidates the latent EVERYWHERE
                try:
                    fp.mailbox.check(collective=True)
                except Exception:
                    fp.mailbox = None  # (released group-wide by check: torch.distributed exchanges from here on)
                    raise
        if precision is not None and isinstance(precision, torch.dtype):
            img = img.to(precision)
        return img, intermediates

    def _partial_guard(self, what):
        if self._multi_rank():
            raise NotImplementedError(f"{what} runs on one GPU (no frame shards, no CFG pair): the ranks of one clip would "
                                      "have to share the encode noise and the start latent")
        if self.multicond:
            raise NotImplementedError(f"{what} is the main sampler's (ddim.py); ddim_multiplecond.py has no such path")

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None, *, fs=None, noise_fn=None, temperature=1.0, guidance_rescale=0.0,
               verbose=True, **kwargs):
        """Denoise `x_latent` from step `t_start` of the current schedule down to the clean latent (ddim.py:292-312): the
        last `t_start` steps of the DDIM loop, `ddim_timesteps[:t_start]` walked backwards - the second half of the img2img
        pair `stochastic_encode(x0, [t_start - 1])` -> `decode(z, cond, t_start)`.  The reference's arguments in its order; the
        keyword-only ones are this sampler's (`noise_fn(i, shape)` as in ddim_sampling; `fs` and **kwargs go to the U-Net - the
        reference's decode passes neither).  Every step is p_sample_ddim: graph replay, the two CFG streams and
        PANDORA_CFG_BATCH apply as in `sample`, and a decode on the tensors a `sample` ran on replays its graph."""
        if use_original_steps:
            raise NotImplementedError(_ORIGINAL_STEPS)
        self._partial_guard("decode")
        total_steps = int(self.ddim_timesteps.shape[0])
        if not 1 <= int(t_start) <= total_steps:
            raise ValueError(f"decode: t_start={t_start} outside [1, {total_steps}] (the schedule's step count)")
        device = self._ops().device
        timesteps = self.ddim_timesteps[:int(t_start)]
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        if verbose:
            from tqdm import tqdm
            iterator = tqdm(time_range, desc="Decoding image", total=total_steps)
        else:
            iterator = time_range
        x_dec = x_latent.to(device=device, dtype=torch.float32).contiguous()  # the loop state stays f32 (see module docstring)
        unet = getattr(getattr(self.model, "model", None), "diffusion_model", None)
        if fs is None and getattr(unet, "fs_condition", False) and hasattr(unet, "default_fs"):
            # the reference's call: no fs, the U-Net falls back to its default_fs (openaimodel3d.py:574-577).  Ours would build that
            # tensor inside every forward - a host-to-device copy, which a graph capture cannot hold - so it is built here, once
            fs = torch.tensor([unet.default_fs], dtype=torch.long, device=device)
        shape = tuple(x_dec.shape)
        for i, step in enumerate(iterator):
            index = total_steps - i - 1
            step = int(step)
            ts = torch.full((shape[0],), step, device=device, dtype=torch.long)
            noise = noise_fn(i, shape) if noise_fn is not None else None
            x_dec, _ = self.p_sample_ddim(x_dec, cond, ts, index, temperature=temperature,
                                          unconditional_guidance_scale=unconditional_guidance_scale,
                                          unconditional_conditioning=unconditional_conditioning, fs=fs, noise=noise,
                                          want_x0=False, step=step, guidance_rescale=guidance_rescale, **kwargs)
            if callback:
                callback(i)
        return x_dec

    def _encode_tables(self, use_original_steps, device):
        """(sqrt(a), sqrt(1 - a)) f32 on `device`, the values the reference forms on the host (ddim.py:318-323, :59): the f32
        square roots of the f32 `ddim_alphas` and of the f32 `1 - ddim_alphas` (_sqrt_f32), or - `use_original_steps` - the f32
        copies of the model's 1000-entry bf16 buffers (:46-47).  Cached until the next make_schedule."""
        key = (bool(use_original_steps), str(device))
        if key not in self._enc_tables:
            if use_original_steps:
                m = self.model
                a = m.sqrt_alphas_cumprod.detach().to(torch.float32).cpu()
                s = m.sqrt_one_minus_alphas_cumprod.detach().to(torch.float32).cpu()
            else:
                a, s = _sqrt_f32(self.ddim_alphas), _sqrt_f32(1.0 - self.ddim_alphas)
            self._enc_tables[key] = (a.contiguous().to(device), s.to(torch.float32).contiguous().to(device))
        return self._enc_tables[key]

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """Noise the clean latent `x0` (b, ...) to step t[b] of the current schedule in one jump (ddim.py:314-328):
        sqrt(a_t) x0 + sqrt(1 - a_t) noise, f32.  `t` (b,) INDEXES the tables - positions in `ddim_timesteps`, or DDPM
        timesteps with `use_original_steps` - it is not a timestep otherwise.  An index outside the table is a ValueError.
        On an op table with `q_sample` (HipOps: pm_q_sample) this is one kernel launch; otherwise the reference's expression
        in torch.  Either way the result equals the reference's bit for bit."""
        self._partial_guard("stochastic_encode")
        ops = self._ops()
        device = ops.device
        tab_a, tab_s = self._encode_tables(use_original_steps, device)
        t = torch.as_tensor(t, dtype=torch.long).reshape(-1)
        x0 = x0.to(device=device, dtype=torch.float32).contiguous()
        if t.shape[0] != x0.shape[0]:
            raise ValueError(f"stochastic_encode: {t.shape[0]} indices for {x0.shape[0]} clips (one per clip)")
        noise = self._draw(tuple(x0.shape), device) if noise is None else noise
        noise = noise.to(device=device, dtype=torch.float32).contiguous()
        q_sample = getattr(ops, "q_sample", None)
        if q_sample is not None:
            return q_sample(x0, noise, t, tab_a, tab_s)
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= tab_a.numel():
            raise ValueError(f"stochastic_encode: indices span [{lo}, {hi}], the tables have {tab_a.numel()} entries")
        idx = t.to(tab_a.device)
        view = (-1,) + (1,) * (x0.dim() - 1)
        return tab_a[idx].view(view) * x0 + tab_s[idx].view(view) * noise


class DDIMSamplerMultiCond(DDIMSampler):
    """The multi-condition sampler (drop-in for lvdm.models.samplers.ddim_multiplecond.DDIMSampler, selected by
    `multiple_cond_cfg=True`, model.py:705): THREE U-Net forwards per step - conditional, unconditional and "image
    tokens + empty text" (`unconditional_conditioning_img_nonetext`, model.py:737-743) - combined as
        v = e_uc + cfg_img (e_uc_img - e_uc) + scale (e_c - e_uc_img)        (ddim_multiplecond.py:233-234)
    with `cfg_img` defaulting to the text scale (:219-220); everything after the combine is the step of the main
    sampler.  In the reference checkout this class is dead on arrival: its make_schedule runs np.sqrt on the bf16
    `alphas_cumprod` buffer and raises TypeError (ddim_multiplecond.py:40; pinned by tests/test_oracle_vs_reference.py).
    The working form - what upstream DynamiCrafter's f32-buffer model runs - is its own sample / ddim_sampling /
    p_sample_ddim on top of the one-line cast the main sampler already has (`alphas_cumprod.to(torch.float32)`,
    ddim.py:27): that recombination of the reference's own code is the parity oracle (oracle/make_golden.py
    gen_ddim_multicond), and this class restates it on the fused update kernel and the three-forward HIP graph."""
    multicond = True
