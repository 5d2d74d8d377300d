"""GPU: `bench.py --gpus 8` rehearsed on the ONE MI355X, launched exactly as the driver launches it (torch.distributed.run,
one process per rank; RANK / LOCAL_RANK / WORLD_SIZE from the environment) - 8 processes sharing the GPU over gloo (one GPU
cannot form an 8-rank RCCL communicator), a U-Net of 64 base channels at the 320x512 latent (`--rehearsal-width`: functional,
not a measurement - the line says so and carries no `value`).  Both 8-GPU decompositions of frame_parallel.make_hybrid:

* hybrid     cond / uncond branch pair x 4 frame shards, temporal blocks re-sharded frames <-> pixels (the default);
* frames-kv  8 frame shards of 2 frames, both branches per rank, K|V all-gather for the temporal attention - the split the
             north-star names (BASELINE configs[3]).

Asserted: the line's shape (metric / n_gpus / scaling), the process group every rank joined, and the exchanges ONE forward
issues on a rank - 105 latency-class exchanges through the peer mailboxes (88 temporal-conv stages + 17 TemporalTransformer
GroupNorms; one kernel launch each, csrc/peer.hip) + 34 bulk collectives (VERDICT r04 #5b).  No reference counterpart
(the reference has no model parallelism)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("split,bulk", [("hybrid", "all_to_all"), ("frames-kv", "gather_kv")])
def test_bench_gpus_8_rehearsal(split, bulk):
    env = dict(os.environ, PANDORA_DIST_BACKEND="gloo", PANDORA_SEGMENT_GRAPHS="force", PANDORA_PEER_TIMEOUT_S="60",
               OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
           "--only", "320x512", "--rehearsal-width", "64", "--split", split, "--full"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1400)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]  # rank 0 prints ONE JSON line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["steps"] == 2 and out["scaling"] == "strong" and out["value"] is None and "rehearsal" in out
    mg = out["multi_gpu"]
    assert mg["rccl_ranks_seen"] == 8 and mg["backend"] == "gloo" and mg["split"] == split and mg["peer_mailbox"] is True
    assert mg["frame_group_world"] == (4 if split == "hybrid" else 8) and mg["cfg_pair"] == (split == "hybrid")
    ex = mg["exchanges_per_forward"]
    assert ex["mailbox"] == 105 and ex["stats_halo"] == 88 and ex["reduce_stats"] == 17, ex
    assert ex[bulk] == 34 and ex["exchange_halo"] == 0, ex
    print(f"\n[scaling] bench.py --gpus 8 rehearsal ({split}, 8 processes on one GPU over gloo, 64-channel U-Net): "
          f"{out['ms_per_step']:.0f} ms/step; per forward {ex['mailbox']:.0f} mailbox launches + {ex[bulk]:.0f} {bulk}")
