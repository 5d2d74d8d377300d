// Host program of tests/test_gemm_walk_cpu.py: the GEMM family's persistent work walk and tile decodes, the very functions
// the kernels call (csrc/gemm_common.hpp: work_item, decode_tile, decode_work), run on the CPU over every grid size the
// launchers can produce.  No HIP API call, no GPU.  Prints one line per failed property and "ok <cases>" at the end; exit
// status 1 on any failure.
#include <stdio.h>
#include <vector>
#include "../open-pandora_amd/csrc/gemm_common.hpp"

using namespace pm;

static long g_failures = 0;
static void fail(const char* what, int a, int b, int c, int d) {
  if (++g_failures <= 20) printf("FAIL %s (%d, %d, %d, %d)\n", what, a, b, c, d);
}

// every work id of [0, nwork) exactly once over all (block, round); no id behind a block's first -1
static void check_walk(int G, int nwork) {
  const int grid = G < nwork ? G : nwork;  // what the launchers ask for
  std::vector<int> seen(nwork, 0);
  for (int bid = 0; bid < grid; ++bid) {
    bool ended = false;
    // (rounds past the last possible one too: a block that ended must stay ended)
    for (int round = 0; round < nwork / grid + 3; ++round) {
      const int w = work_item(bid, grid, nwork, round);
      if (w < -1 || w >= nwork) {  // bounds first: `seen` is indexed with it
        fail("work id out of range", G, nwork, bid, round);
        continue;
      }
      if (w < 0) {
        ended = true;
        continue;
      }
      if (ended) fail("work id behind the block's first -1", G, nwork, bid, round);
      ++seen[w];
    }
  }
  for (int w = 0; w < nwork; ++w)
    if (seen[w] != 1) fail(seen[w] ? "work id repeated" : "work id missed", G, nwork, w, seen[w]);
}

static void check_decode_tile(int mtiles, int ntiles) {
  std::vector<int> seen(mtiles * ntiles, 0);
  for (int w = 0; w < mtiles * ntiles; ++w) {
    int mt = -1, nt = -1;
    decode_tile(mtiles, ntiles, w, mt, nt);
    if (mt < 0 || mt >= mtiles || nt < 0 || nt >= ntiles)
      fail("decode_tile out of the grid", mtiles, ntiles, w, mt);
    else
      ++seen[mt * ntiles + nt];
  }
  for (int t = 0; t < mtiles * ntiles; ++t)
    if (seen[t] != 1) fail("decode_tile not a bijection", mtiles, ntiles, t, seen[t]);
}

template <int AMODE, int TILE_ROWS> static void check_decode_work(int mtiles, int ntiles, int splits) {
  GemmParams p{};
  p.mtiles = mtiles;
  p.ntiles = ntiles;
  p.splits = splits;
  // temporal mode: F frames of P pixels with whole tiles per frame, so that the pixel-block-major remap is taken when
  // mtiles is a multiple of 4 frames (and not taken otherwise)
  p.F = 4;
  p.P = TILE_ROWS * (mtiles % 4 == 0 ? mtiles / 4 : 1);
  const int n = mtiles * ntiles * splits;
  std::vector<int> seen(n, 0);
  for (int w = 0; w < n; ++w) {
    int mt = -1, nt = -1, split = -1;
    decode_work<AMODE, TILE_ROWS>(p, w, mt, nt, split);
    if (mt < 0 || mt >= mtiles || nt < 0 || nt >= ntiles || split < 0 || split >= splits)
      fail("decode_work out of the grid", mtiles, ntiles, splits, w);
    else
      ++seen[(mt * ntiles + nt) * splits + split];
  }
  for (int t = 0; t < n; ++t)
    if (seen[t] != 1) fail("decode_work not a bijection", mtiles, ntiles, splits, t);
}

int main() {
  long cases = 0;
  const int grids[] = {1, 7, 8, 64, 255, 256, 304};
  for (int G : grids)
    for (int nwork = 1; nwork <= 1200; ++nwork, ++cases) check_walk(G, nwork);
  for (int mtiles = 1; mtiles <= 40; ++mtiles)
    for (int ntiles = 1; ntiles <= 20; ++ntiles) {
      check_decode_tile(mtiles, ntiles);
      ++cases;
      for (int splits = 1; splits <= 4; ++splits, cases += 3) {
        check_decode_work<A_DENSE, 128>(mtiles, ntiles, splits);
        check_decode_work<A_CONVT3, 128>(mtiles, ntiles, splits);
        check_decode_work<A_CONVT3, 256>(mtiles, ntiles, splits);
      }
    }
  if (g_failures) {
    printf("%ld failures\n", g_failures);
    return 1;
  }
  printf("ok %ld\n", cases);
  return 0;
}
