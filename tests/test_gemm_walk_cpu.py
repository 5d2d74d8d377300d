"""The GEMM family's persistent work walk and tile decodes on the CPU: tests/gemm_walk_check.hip is a stand-alone host program
(its own main, no HIP API call, never loaded into python) that includes csrc/gemm_common.hpp and calls the very work_item /
decode_tile / decode_work the kernels call.  For G in {1, 7, 8, 64, 255, 256, 304} and nwork = 1..1200 with grid = min(G, nwork):
every work id is produced exactly once over all (block, round) and no block produces an id behind its first -1 (the program
bounds-checks every id before it indexes with it); decode_tile is a bijection onto the tile grid for mtiles 1..40 x ntiles
1..20; decode_work is a bijection onto (row tile, column tile, split) for splits 1..4, with and without the temporal mode's
pixel-block-major remap."""
import os
import subprocess

from open_pandora_amd import build as _b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_work_walk_and_tile_decodes_are_bijections(tmp_path):
    exe = str(tmp_path / "gemm_walk_check")
    # host side only: the program launches nothing, so no device code is compiled for it
    subprocess.run([_b._hipcc(), "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-Wno-unused-result",
                    os.path.join(ROOT, "tests", "gemm_walk_check.hip"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # 7 grids x 1200 work counts + 800 tile grids x (1 + 4 splits x 3 decode_work forms)
    assert r.stdout.split()[-2:] == ["ok", str(7 * 1200 + 800 * 13)]
