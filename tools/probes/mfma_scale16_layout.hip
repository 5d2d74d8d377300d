// Operand AND scale lane map of v_mfma_scale_f32_16x16x128_f8f6f4 with fp8 (e4m3) A and B (the form pm_gemm_mx8 runs on):
// exact small integers with a DIFFERENT E8M0 scale per lane, i.e. per (row, 32-block of K) for A and per (column, block) for
// B, so that a scale applied to the wrong block or row shows.  Hypothesis 0: lane l holds row l & 15, k = 32 (l >> 4) + idx
// (idx = byte 0..31 of its 8 VGPRs) and its scale operand scales that same (row, block).  Hypothesis 1: two K = 64 halves,
// k = 16 (l >> 4) + (idx & 15) + 64 (idx >> 4), the scale of lane l for block l >> 4.  Then: does a NaN scale (0xFF) or a
// NaN element (0x7F) make the product NaN?
// Result on MI355X: hypothesis 1 (0 / 256 mismatches; hypothesis 0: 255 / 256), and both a 0xFF scale and NaN elements turn
// exactly the 16 outputs of that row of A into NaN (the per-row counts below index the output column, l & 15, not the row).
//   build: hipcc --offload-arch=gfx950 -O2 mfma_scale16_layout.hip -o probe16
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
typedef __attribute__((ext_vector_type(8))) int v8i;
typedef __attribute__((ext_vector_type(4))) float v4f;
__global__ void k(const int* a, const int* b, const int* sa, const int* sb, float* c) {
  v8i A, B;
  for (int i = 0; i < 8; ++i) {
    A[i] = a[threadIdx.x * 8 + i];
    B[i] = b[threadIdx.x * 8 + i];
  }
  v4f C = {0.f, 0.f, 0.f, 0.f};
  C = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, B, C, 0, 0, 0, sa[threadIdx.x], 0, sb[threadIdx.x]);
  for (int i = 0; i < 4; ++i) c[threadIdx.x * 4 + i] = C[i];
}
static unsigned char enc(int v) {  // e4m3 of a small integer in [-3, 3]
  static const unsigned char t[4] = {0x00, 0x38, 0x40, 0x44};
  return v < 0 ? (unsigned char)(t[-v] | 0x80) : t[v];
}
static int kmap(int hyp, int g, int idx) { return hyp == 0 ? 32 * g + idx : 16 * g + (idx & 15) + 64 * (idx >> 4); }
int main() {
  static int A[16][128], B[128][16], SA[16][4], SB[16][4];
  srand(11);
  for (int i = 0; i < 16; ++i)
    for (int q = 0; q < 128; ++q) A[i][q] = rand() % 7 - 3;
  for (int q = 0; q < 128; ++q)
    for (int j = 0; j < 16; ++j) B[q][j] = rand() % 7 - 3;
  for (int i = 0; i < 16; ++i)
    for (int g = 0; g < 4; ++g) {
      SA[i][g] = 127 + (i * 4 + g) % 7 - 3;  // 2^-3 .. 2^3
      SB[i][g] = 127 + (i * 3 + 2 * g) % 5 - 2;
    }
  double want[16][16];
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j) {
      double s = 0;
      for (int q = 0; q < 128; ++q) s += A[i][q] * ldexp(1.0, SA[i][q / 32] - 127) * B[q][j] * ldexp(1.0, SB[j][q / 32] - 127);
      want[i][j] = s;
    }
  int *da, *db, *dsa, *dsb;
  float* dc;
  hipMalloc(&da, 64 * 32);
  hipMalloc(&db, 64 * 32);
  hipMalloc(&dsa, 64 * 4);
  hipMalloc(&dsb, 64 * 4);
  hipMalloc(&dc, 64 * 4 * 4);
  int found = -1;
  for (int hyp = 0; hyp < 2; ++hyp) {
    unsigned char ha[64][32], hb[64][32];
    int hsa[64], hsb[64];
    for (int l = 0; l < 64; ++l) {
      for (int idx = 0; idx < 32; ++idx) {
        const int kk = kmap(hyp, l >> 4, idx);
        ha[l][idx] = enc(A[l & 15][kk]);
        hb[l][idx] = enc(B[kk][l & 15]);
      }
      hsa[l] = SA[l & 15][l >> 4];
      hsb[l] = SB[l & 15][l >> 4];
    }
    hipMemcpy(da, ha, sizeof(ha), hipMemcpyHostToDevice);
    hipMemcpy(db, hb, sizeof(hb), hipMemcpyHostToDevice);
    hipMemcpy(dsa, hsa, sizeof(hsa), hipMemcpyHostToDevice);
    hipMemcpy(dsb, hsb, sizeof(hsb), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dc);
    float hc[64][4];
    hipMemcpy(hc, dc, sizeof(hc), hipMemcpyDeviceToHost);
    int bad = 0;
    for (int l = 0; l < 64; ++l)
      for (int r = 0; r < 4; ++r) bad += hc[l][r] != (float)want[4 * (l >> 4) + r][l & 15];  // C/D: row 4 (l >> 4) + r, col l & 15
    printf("hypothesis %d: %d / 256 mismatches%s\n", hyp, bad, bad ? "" : "   <== operand and scale map");
    if (!bad && found < 0) found = hyp;
    if (!bad) {
      // NaN propagation: row 3 of A with scale 0xFF (elements finite), then row 5 with NaN elements (scale finite)
      hsa[3] = 0xff;
      hipMemcpy(dsa, hsa, sizeof(hsa), hipMemcpyHostToDevice);
      hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dc);
      hipMemcpy(hc, dc, sizeof(hc), hipMemcpyDeviceToHost);
      int nan_row = 0, nan_other = 0;
      for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) (l & 15) == 3 ? nan_row += std::isnan(hc[l][r]) : nan_other += std::isnan(hc[l][r]);
      printf("scale 0xFF on row 3 of A: %d / 16 NaN in that row, %d NaN elsewhere\n", nan_row, nan_other);
      hsa[3] = SA[3][0];
      for (int idx = 0; idx < 32; ++idx) ha[5][idx] = 0x7f;
      hipMemcpy(dsa, hsa, sizeof(hsa), hipMemcpyHostToDevice);
      hipMemcpy(da, ha, sizeof(ha), hipMemcpyHostToDevice);
      hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dc);
      hipMemcpy(hc, dc, sizeof(hc), hipMemcpyDeviceToHost);
      nan_row = nan_other = 0;
      for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) (l & 15) == 5 ? nan_row += std::isnan(hc[l][r]) : nan_other += std::isnan(hc[l][r]);
      printf("e4m3 NaN elements in row 5 of A: %d / 16 NaN in that row, %d NaN elsewhere\n", nan_row, nan_other);
    }
  }
  return found >= 0 ? 0 : 1;
}
