// 2-D Winograd F(2x2,3x3) convolution on fp32 MFMA for the stride-1, "same"-padded dense 3x3
// convolutions of the decoders and the merged heads (forward AND data gradient).
//
//   Y = A^T [ sum_c U2(c) .* V(c) ] A      V = B^T d B  (d = the 4x4 input patch of a 2x2 output
//                                          tile, rows / columns 2t-1 .. 2t+2),  U2 = G g G^T
//   B^T rows: (d0-d2, d1+d2, d2-d1, d1-d3)     A^T = (1 1 1 0; 0 1 -1 -1)
// 16 GEMMs over a QUARTER of the pixels: 16 of the 36 direct-convolution multiplies per output
// tile, where the row form of conv_wino.hip (F(2,3) along W, kernel rows in the GEMM K) runs 24.
//
// Workgroup = 32 output tiles (consecutive in (image, tile row, tile column) order, may wrap lines
// and images) x 32*NT output channels, 4 waves: wave j owns column component j and ALL four row
// components (4*NT accumulator tiles of 32x32).  The transform is separable:
//   * the ROW direction is applied once per element where the prefetched raw patch rows leave their
//     registers for LDS (a loader thread holds the four rows of one (tile, patch column, float4):
//     four packed adds / subtracts per row component), staged as Hs[4 i][4 col][32 tiles][8];
//   * the COLUMN direction stays in the consuming wave, as in the row kernel: operand = sum /
//     difference of two ds_read_b128.
// K step = 8 channels, LDS rows of 32 B ([row][8]; a [half][row][4] image without the 2-way read
// conflict measured 5-15 % SLOWER: its loader lanes fetch 16 scattered bytes each instead of 32).
// U2 lives in memory as [comp][K step][n][8], so a wave's U loads of a step are contiguous.
// Single LDS buffer + register prefetch.  The K summation runs over the channels in order,
// whatever the tile's position or the batch size.  The epilogue applies the row
// output transform in registers, transposes through LDS in two halves (output row 0 / 1 of the
// tiles) and continues exactly like conv1d_wino_kernel (column output transform, bias, BatchNorm
// statistics partials, folded BatchNorm, residual, ReLU-backward mask, ReLU; 16-B stores).
#include "common.h"
#include "prof.h"

namespace {

constexpr int kK2 = 8;            // channels per K step
constexpr int kTiles = 32;        // 2x2 output tiles per workgroup

typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
typedef float vf32x2 __attribute__((ext_vector_type(2)));
constexpr uint32_t kOOBw = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t vrsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 vbuf_ld4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}
__device__ __forceinline__ float4 vbuf_ld4s(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(float4,
                            __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ uint32_t vdiv(uint32_t n, uint32_t mul, uint32_t sh) {
  return (__umulhi(n, mul) + n) >> sh;
}
__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
  const vf32x2 lo = vf32x2{a.x, a.y} - vf32x2{b.x, b.y}, hi = vf32x2{a.z, a.w} - vf32x2{b.z, b.w};
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  const vf32x2 lo = vf32x2{a.x, a.y} + vf32x2{b.x, b.y}, hi = vf32x2{a.z, a.w} + vf32x2{b.z, b.w};
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}

struct Wino2dArgs {
  const float* in;
  const float* u;                   // U2 [16][ksteps][n_ch][8]
  float* out;
  const float* bias;
  float* stats;                     // [3][tiles_m][n_ch]: sum, M2 about the tile mean, count
  const float* scale;
  const float* shift;
  const float* residual;
  const float* mask_src;
  int ld_out, ld_res, ld_mask, act;
  int H, W, TH, TW, MT;             // image size, tiles per column / line, total tiles
  int k_ch, n_ch;
  int in_simg, in_srow, in_spx;     // input element strides
  int tiles_m, tiles_n, ksteps;
  uint32_t in_bytes, u_bytes;
  uint32_t mul_tw, sh_tw, mul_th, sh_th;   // magic division by TW and by TH
};

template <int NT>   // accumulator tiles of 32 channels per row component: workgroup = 32 * NT channels
__global__ __launch_bounds__(256, NT == 1 ? 4 : 2) void conv_wino2d_kernel(const Wino2dArgs p) {
  constexpr int WN = 32 * NT;
  constexpr int NC4 = WN / 4;                     // float4 columns of a tile row
  constexpr int RG = 256 / NC4;                   // pixel rows covered by one pass of the block
  constexpr int PXH = 64 / RG;                    // output pixels per thread and half
  constexpr int PXI = 2 * PXH;
  constexpr int BLD = 16 * WN * 2 / 256;          // U float4 loads per thread and K step
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const Hs = smem;                          // [4 i][4 col][32 tiles][8]
  float* const Us = smem + 16 * kTiles * kK2;      // [16 comps][WN][8]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const int wg = emsa_xcd_remap(blockIdx.x, gridDim.x);
  const int nt = wg % p.tiles_n, mt = wg / p.tiles_n;
  const int q0 = mt * kTiles, n0 = nt * WN;
  const __amdgpu_buffer_rsrc_t rs_in = vrsrc(p.in, p.in_bytes);
  const __amdgpu_buffer_rsrc_t rs_u = vrsrc(p.u, p.u_bytes);

  // ---- loader state (fixed for the tile) ---------------------------------------------------------
  // A: thread = (float4 chunk, tile, patch column = wave): the four patch rows -> 4 loads;
  // B: 16 comps x WN channels x 2 chunks -> BLD loads.  Every address = per-thread byte offset +
  // a wave-uniform K offset in the instruction's scalar-offset operand.
  const int c4 = (tid & 1) * 4;
  const int ltile = (tid >> 1) & 31;
  uint32_t a_voff[4], b_voff[BLD];
  {
    const int q = q0 + ltile;
    int base = 0, y0 = 0;                             // element offset of patch row 1 (y = 2 ty)
    bool xok = false;
    if (q < p.MT) {
      const int line = (int)vdiv((uint32_t)q, p.mul_tw, p.sh_tw);       // img * TH + ty
      const int tx = q - line * p.TW;
      const int img = (int)vdiv((uint32_t)line, p.mul_th, p.sh_th);
      const int ty = line - img * p.TH;
      const int x = 2 * tx - 1 + wave;
      y0 = 2 * ty;
      xok = x >= 0 && x < p.W;
      base = img * p.in_simg + y0 * p.in_srow + x * p.in_spx + c4;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int y = y0 + r - 1;
      const bool ok = xok && y >= 0 && y < p.H;
      // a row above / below the image or a column past a line end reads zero: its offset leaves
      // the descriptor's range instead of aliasing the neighbouring line or image
      a_voff[r] = ok ? (uint32_t)(base + (r - 1) * p.in_srow) * 4u : kOOBw;
    }
  }
#pragma unroll
  for (int j = 0; j < BLD; ++j) {
    const int f = (tid >> 1) + 128 * j;               // 0..16*WN-1 = comp * WN + n
    const int comp = f / WN, n = n0 + (f % WN);
    // U2 is laid out [comp][K step][n][8]: a wave's 32 rows of a K step are 1 KiB contiguous
    b_voff[j] = n < p.n_ch ? (uint32_t)((comp * p.ksteps * p.n_ch + n) * kK2 + c4) * 4u : kOOBw;
  }
  // kOOBw for the lanes whose channels lie beyond k_ch in the LAST K step
  const uint32_t last_oob = (p.ksteps - 1) * kK2 + c4 < p.k_ch ? 0u : kOOBw;
  float4 ra[4], rb[BLD];
  auto load_regs = [&](int s) {
    const uint32_t so = (uint32_t)(s * kK2) * 4u, sou = (uint32_t)(s * p.n_ch * kK2) * 4u;
    // one v_and_or per load with a wave-uniform mask, not a branch around the loads
    const uint32_t pm = (s + 1) * kK2 > p.k_ch ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) ra[r] = vbuf_ld4s(rs_in, a_voff[r] | (last_oob & pm), so);
#pragma unroll
    for (int j = 0; j < BLD; ++j) rb[j] = vbuf_ld4s(rs_u, b_voff[j] | (last_oob & pm), sou);
  };
  auto store_lds = [&]() {
    // row transform B^T on the way to LDS; a wave writes 1 KiB contiguously per component
    float* const h = Hs + (wave * kTiles + ltile) * kK2 + c4;
    emsa_st4(h + 0 * 4 * kTiles * kK2, sub4(ra[0], ra[2]));
    emsa_st4(h + 1 * 4 * kTiles * kK2, add4(ra[1], ra[2]));
    emsa_st4(h + 2 * 4 * kTiles * kK2, sub4(ra[2], ra[1]));
    emsa_st4(h + 3 * 4 * kTiles * kK2, sub4(ra[1], ra[3]));
#pragma unroll
    for (int j = 0; j < BLD; ++j) emsa_st4(Us + ((tid >> 1) + 128 * j) * kK2 + c4, rb[j]);
  };

  // wave j: V_ij = Hs[i][ca] + sg * Hs[i][cb]
  const int ca = wave == 0 ? 0 : wave == 2 ? 2 : 1;
  const int cb = wave == 2 ? 1 : wave == 3 ? 3 : 2;
  const float sg = wave == 1 ? 1.f : -1.f;

  load_regs(0);
  f32x16 acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][t][r] = 0.f;
  store_lds();
  __syncthreads();
  const float* const a0 = Hs + (ca * kTiles + l31) * kK2 + lh * 4;
  const float* const a1 = Hs + (cb * kTiles + l31) * kK2 + lh * 4;
  const float* const b = Us + (wave * WN + l31) * kK2 + lh * 4;
  for (int s = 0; s < p.ksteps; ++s) {
    const bool has_next = s + 1 < p.ksteps;
    __builtin_amdgcn_s_setprio(3);           // the next step's loads go out first
    if (has_next) load_regs(s + 1);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 x0 = emsa_ld4(a0 + i * 4 * kTiles * kK2), x1 = emsa_ld4(a1 + i * 4 * kTiles * kK2);
      const vf32x2 sg2 = {sg, sg};
      const vf32x2 vlo = __builtin_elementwise_fma(vf32x2{x1.x, x1.y}, sg2, vf32x2{x0.x, x0.y});
      const vf32x2 vhi = __builtin_elementwise_fma(vf32x2{x1.z, x1.w}, sg2, vf32x2{x0.z, x0.w});
      float4 fb[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u) fb[u] = emsa_ld4(b + (i * 4 * WN + u * 32) * kK2);
#pragma unroll
      for (int u = 0; u < NT; ++u)
        acc[i][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(vlo.x, fb[u].x, acc[i][u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < NT; ++u)
        acc[i][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(vlo.y, fb[u].y, acc[i][u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < NT; ++u)
        acc[i][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(vhi.x, fb[u].z, acc[i][u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < NT; ++u)
        acc[i][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(vhi.y, fb[u].w, acc[i][u], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    if (has_next) store_lds();
    __syncthreads();
  }

  // ---- epilogue ------------------------------------------------------------------------------------
  // half a = output row a of every tile: the wave forms T_a = A^T (row direction) of its four
  // accumulators in registers and stages it as [4 j][32 tiles][WN + 4]; thread (px = tid / NC4 + RG*k,
  // col4 = tid % NC4) owns PXH of the half's 64 pixels (tile * 2 + b) x one float4 of channels
  constexpr int SLD = WN + 4;
  constexpr uint32_t kNoPix = 0xFFFFFFFFu;
  float* const stage = smem;
  const int col4 = tid % NC4, n = n0 + col4 * 4;
  const int rgi = tid / NC4;
  const bool nok = n < p.n_ch;
  // lane l of every wave: pixel index of output (tile l / 2, row a, column l % 2)
  uint32_t lane_pix[2] = {kNoPix, kNoPix};
  {
    const int q = q0 + (lane >> 1);
    if (q < p.MT) {
      const int line = (int)vdiv((uint32_t)q, p.mul_tw, p.sh_tw);
      const int tx = q - line * p.TW;
      const int img = (int)vdiv((uint32_t)line, p.mul_th, p.sh_th);
      const int ty = line - img * p.TH;
      const int x = 2 * tx + (lane & 1);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int y = 2 * ty + a;
        // the virtual row / column of an odd size is computed and never stored
        if (x < p.W && y < p.H) lane_pix[a] = (uint32_t)((img * p.H + y) * p.W + x);
      }
    }
  }
  vf32x2 ylo[PXI], yhi[PXI];
  uint32_t opix[PXI];          // pixel index (< 2^29, checked by the launcher)
  bool ok[PXI];
  const float4 bv = (nok && p.bias) ? emsa_ld4(p.bias + n) : emsa_zero4();
  const vf32x2 blo = {bv.x, bv.y}, bhi = {bv.z, bv.w};
  // out(b=0) = m0 + m1 + m2, out(b=1) = m1 - m2 - m3  ==  m1 + sg * (m2 + m03); b = px & 1 is a
  // per-thread constant (RG is even)
  const float sgo = (rgi & 1) ? -1.f : 1.f;
  const vf32x2 sg2o = {sgo, sgo};
  const int m03row = (rgi & 1) ? 3 : 0;
#pragma unroll
  for (int k = 0; k < PXI; ++k) {
    const int a = k / PXH, kk = k % PXH;
    const uint32_t o = (uint32_t)__builtin_amdgcn_ds_bpermute((rgi + RG * kk) * 4, (int)lane_pix[a]);
    ok[k] = nok && o != kNoPix;
    opix[k] = o;
  }
  // every tensor touched by the epilogue is < 2 GiB (checked by the launcher): an offset with the
  // top bit set is out of range -- loads return zero, stores are dropped
  const __amdgpu_buffer_rsrc_t rs_out = vrsrc(p.out, kOOBw);
  const __amdgpu_buffer_rsrc_t rs_res = vrsrc(p.residual, kOOBw);
  const __amdgpu_buffer_rsrc_t rs_msk = vrsrc(p.mask_src, kOOBw);
  // all the epilogue's loads are issued here, before the accumulators are staged through LDS
  float4 rres[PXI], rmsk[PXI];
#pragma unroll
  for (int k = 0; k < PXI; ++k) {
    const bool live = ok[k];
    if (p.residual)
      rres[k] = vbuf_ld4(rs_res, live ? (opix[k] * (uint32_t)p.ld_res + (uint32_t)n) * 4u : kOOBw);
    if (p.mask_src)
      rmsk[k] = vbuf_ld4(rs_msk, live ? (opix[k] * (uint32_t)p.ld_mask + (uint32_t)n) * 4u : kOOBw);
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    __syncthreads();                     // the K loop's buffers / half 0 of the stage are consumed
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float v = a == 0 ? (acc[0][t][r] + acc[1][t][r]) + acc[2][t][r]
                               : (acc[1][t][r] - acc[2][t][r]) - acc[3][t][r];
        stage[(wave * kTiles + row) * SLD + t * 32 + l31] = v;
      }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < PXH; ++kk) {
      const int k = a * PXH + kk;
      const int tl = (rgi + RG * kk) >> 1;           // tile of this pixel
      const float4 m1 = emsa_ld4(stage + (1 * kTiles + tl) * SLD + col4 * 4);
      const float4 m2 = emsa_ld4(stage + (2 * kTiles + tl) * SLD + col4 * 4);
      const float4 m03 = emsa_ld4(stage + (m03row * kTiles + tl) * SLD + col4 * 4);
      const vf32x2 tlo = vf32x2{m2.x, m2.y} + vf32x2{m03.x, m03.y};
      const vf32x2 thi = vf32x2{m2.z, m2.w} + vf32x2{m03.z, m03.w};
      ylo[k] = __builtin_elementwise_fma(tlo, sg2o, vf32x2{m1.x, m1.y}) + blo;
      yhi[k] = __builtin_elementwise_fma(thi, sg2o, vf32x2{m1.z, m1.w}) + bhi;
    }
  }

  if (p.stats != nullptr) {
    // per-workgroup (sum, M2 about the workgroup's mean, count) over its VALID output pixels: the
    // rows bn_finalize_rows_kernel merges
    __syncthreads();                               // everyone has read `stage`
    float* red = smem;                             // [RG row groups][WN]
    float* tmean = smem + RG * WN;                 // [WN]
    int* scnt = reinterpret_cast<int*>(tmean + WN);    // [RG] valid pixels per row group
    vf32x2 s1lo = {0.f, 0.f}, s1hi = {0.f, 0.f};
    float wgt[PXI];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < PXI; ++k) {
      wgt[k] = ok[k] ? 1.f : 0.f;
      const vf32x2 w2 = {wgt[k], wgt[k]};
      s1lo = __builtin_elementwise_fma(ylo[k], w2, s1lo);
      s1hi = __builtin_elementwise_fma(yhi[k], w2, s1hi);
      cnt += ok[k] ? 1 : 0;
    }
    emsa_st4(red + rgi * WN + col4 * 4, make_float4(s1lo.x, s1lo.y, s1hi.x, s1hi.y));
    // the valid-pixel count is the same for every channel column: column 0 threads publish it
    // (n0 < n_ch for every launched tile, so their `ok` flags are the pixel validity)
    if (col4 == 0) scnt[rgi] = cnt;
    __syncthreads();
    if (tid < WN) {
      float a1 = 0.f;
#pragma unroll
      for (int g = 0; g < RG; ++g) a1 += red[g * WN + tid];
      int c = 0;
#pragma unroll
      for (int g = 0; g < RG; ++g) c += scnt[g];
      tmean[tid] = c > 0 ? a1 / (float)c : 0.f;
      if (n0 + tid < p.n_ch) {
        p.stats[((size_t)0 * p.tiles_m + mt) * p.n_ch + n0 + tid] = a1;
        p.stats[((size_t)2 * p.tiles_m + mt) * p.n_ch + n0 + tid] = (float)c;
      }
    }
    __syncthreads();
    const float4 mu = emsa_ld4(tmean + col4 * 4);
    const vf32x2 mulo = {mu.x, mu.y}, muhi = {mu.z, mu.w};
    vf32x2 s2lo = {0.f, 0.f}, s2hi = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < PXI; ++k) {
      const vf32x2 w2 = {wgt[k], wgt[k]};
      const vf32x2 dlo = ylo[k] - mulo, dhi = yhi[k] - muhi;
      s2lo = __builtin_elementwise_fma(dlo * w2, dlo, s2lo);
      s2hi = __builtin_elementwise_fma(dhi * w2, dhi, s2hi);
    }
    __syncthreads();
    emsa_st4(red + rgi * WN + col4 * 4, make_float4(s2lo.x, s2lo.y, s2hi.x, s2hi.y));
    __syncthreads();
    if (tid < WN && n0 + tid < p.n_ch) {
      float a2 = 0.f;
#pragma unroll
      for (int g = 0; g < RG; ++g) a2 += red[g * WN + tid];
      p.stats[((size_t)1 * p.tiles_m + mt) * p.n_ch + n0 + tid] = a2;
    }
  }

  {
    vf32x2 sclo = {1.f, 1.f}, schi = {1.f, 1.f}, shlo = {0.f, 0.f}, shhi = {0.f, 0.f};
    const bool affine = p.scale != nullptr;
    if (affine && nok) {
      const float4 sc = emsa_ld4(p.scale + n), sh = emsa_ld4(p.shift + n);
      sclo = vf32x2{sc.x, sc.y}; schi = vf32x2{sc.z, sc.w};
      shlo = vf32x2{sh.x, sh.y}; shhi = vf32x2{sh.z, sh.w};
    }
#pragma unroll
    for (int k = 0; k < PXI; ++k) {
      const bool live = ok[k];
      vf32x2 vlo = ylo[k], vhi = yhi[k];
      if (affine) {
        vlo = __builtin_elementwise_fma(vlo, sclo, shlo);
        vhi = __builtin_elementwise_fma(vhi, schi, shhi);
      }
      if (p.residual) {
        vlo += vf32x2{rres[k].x, rres[k].y};
        vhi += vf32x2{rres[k].z, rres[k].w};
      }
      float4 v = make_float4(vlo.x, vlo.y, vhi.x, vhi.y);
      if (p.mask_src) {
        const float4 mm = rmsk[k];
        v.x = mm.x > 0.f ? v.x : 0.f; v.y = mm.y > 0.f ? v.y : 0.f;
        v.z = mm.z > 0.f ? v.z : 0.f; v.w = mm.w > 0.f ? v.w : 0.f;
      }
      if (p.act == EMSA_ACT_RELU) {
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f);
        v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
      }
      const uint32_t off = live ? (opix[k] * (uint32_t)p.ld_out + (uint32_t)n) * 4u : kOOBw;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), rs_out, (int)off, 0, 0);
    }
  }
}

// U2 (emsa_wino2d_at: [16][K step][n][8]) from OIHW weights [co][ci][3][3]: forward (n = cout, k = cin) and/or data gradient
// (n = cin, k = cout, kernel flipped in both directions = components 0 <-> 3 swapped)
__global__ void pack_wino2d_kernel(const float* __restrict__ w, float* __restrict__ u,
                                   float* __restrict__ ud, int cout, int cin) {
  const int total = cout * cin;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int ci = i % cin, co = i / cin;
    float g[9], v[16];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = w[(size_t)i * 9 + t];
    emsa_wino2d_u(g, v);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      if (u) u[emsa_wino2d_at(c, co, ci, cout, cin)] = v[c];
      if (ud) ud[emsa_wino2d_at(emsa_wino2d_flip(c), ci, co, cin, cout)] = v[c];
    }
  }
}

// same transform from the PACKED implicit-GEMM layout wp[tap = r*3 + t][n][k]; flip = 1 for the
// data-gradient pack ([tap][cin][cout], taps not flipped there) -> kernel flipped here
__global__ void pack_wino2d_packed_kernel(const float* __restrict__ wp, float* __restrict__ u,
                                          int n, int k, int flip) {
  const int total = n * k;
  const size_t NK = (size_t)total;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    float g[9], v[16];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = wp[(size_t)(flip ? 8 - t : t) * NK + i];
    emsa_wino2d_u(g, v);
#pragma unroll
    for (int c = 0; c < 16; ++c) u[emsa_wino2d_at(c, i / k, i % k, n, k)] = v[c];
  }
}

inline void magic2(uint32_t d, uint32_t& mul, uint32_t& sh) {
  uint32_t s = 0;
  while ((1ull << s) < d) ++s;
  sh = s;
  mul = (uint32_t)(((1ull << 32) * ((1ull << s) - d)) / d + 1);
}

}  // namespace

extern "C" int emsa_pack_wino2d(const float* w_oihw, float* u, float* u_dgrad, int32_t cout,
                                int32_t cin, void* stream) {
  if (!w_oihw || (!u && !u_dgrad)) return EMSA_E_ARG;
  if (cout < 1 || cin < 1) return EMSA_E_SHAPE;
  int grid = (cout * cin + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(pack_wino2d_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w_oihw, u,
                     u_dgrad, cout, cin);
  return emsa_launch_status();
}

extern "C" int emsa_pack_wino2d_packed(const float* w_packed, float* u, int32_t n_ch, int32_t k_ch,
                                       int32_t flip, void* stream) {
  if (!w_packed || !u) return EMSA_E_ARG;
  if (n_ch < 1 || k_ch < 1) return EMSA_E_SHAPE;
  int grid = (n_ch * k_ch + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(pack_wino2d_packed_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                     w_packed, u, n_ch, k_ch, flip ? 1 : 0);
  return emsa_launch_status();
}

// 1 if `g` (forward or data-gradient geometry of a conv) is a dense stride-1 3x3 "same" conv on
// tensors the kernel's 32-bit offsets reach
extern "C" int emsa_conv_wino2d_supported(const EmsaConvGeom* g) {
  if (!g) return 0;
  if (g->out_pix_img || g->out_pix_row || g->out_pix_px || g->out_pix_off) return 0;
  // forward geometry: off = -1, step = +1; data gradient: off = +1, step = -1
  auto tap3 = [](int off, int step) { return (off == -1 || off == 1) && step == -off; };
  if (!(g->kh == 3 && g->kw == 3 && tap3(g->off_w, g->step_w) && tap3(g->off_h, g->step_h) &&
        g->off_h == g->off_w))
    return 0;
  if (g->mul_h != 1 || g->mul_w != 1 || g->div_h != 1 || g->div_w != 1) return 0;
  if (g->n_img < 1 || g->in_h < 1 || g->in_w < 1 || g->k_ch < 4 || g->n_ch < 4) return 0;
  if (g->in_h != g->out_h || g->in_w != g->out_w) return 0;
  if ((g->k_ch & 3) || (g->n_ch & 3) || (g->ld_out & 3) || (g->in_px_stride & 3) ||
      (g->in_row_stride & 3) || (g->in_img_stride & 3))
    return 0;
  if ((long)g->n_img * g->in_img_stride >= (1L << 29)) return 0;
  if ((long)16 * g->n_ch * (g->k_ch + 7) >= (1L << 29)) return 0;
  return 1;
}

extern "C" int emsa_conv_wino2d_stats_rows(const EmsaConvGeom* g) {
  if (!emsa_conv_wino2d_supported(g)) return EMSA_E_SHAPE;
  const long mtl = (long)g->n_img * ((g->out_h + 1) / 2) * ((g->out_w + 1) / 2);
  return (int)((mtl + kTiles - 1) / kTiles);
}

extern "C" int emsa_conv_wino2d(const EmsaConvGeom* g, const float* in, const float* u2, float* out,
                                const float* bias, float* stats, const float* scale,
                                const float* shift, const float* residual, int32_t ld_res,
                                const float* mask_src, int32_t ld_mask, int32_t act,
                                void* stream) {
  if (!emsa_conv_wino2d_supported(g)) return EMSA_E_SHAPE;
  if (!in || !u2 || !out) return EMSA_E_ARG;
  if ((scale == nullptr) != (shift == nullptr)) return EMSA_E_ARG;
  // operand combinations the epilogue does not take: statistics are those of the conv's own
  // result (+ bias) -- not of a rescaled, masked or activated one
  if (stats && (scale || residual || mask_src || act != EMSA_ACT_NONE)) return EMSA_E_SHAPE;
  if (act != EMSA_ACT_NONE && act != EMSA_ACT_RELU) return EMSA_E_SHAPE;
  auto al16 = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  if (!al16(in) || !al16(u2) || !al16(out) || !al16(bias) || !al16(scale) || !al16(shift) ||
      (residual && (!al16(residual) || (ld_res & 3))) ||
      (mask_src && (!al16(mask_src) || (ld_mask & 3))))
    return EMSA_E_SHAPE;
  Wino2dArgs a;
  a.in = in; a.u = u2; a.out = out; a.bias = bias; a.stats = stats; a.scale = scale;
  a.shift = shift; a.residual = residual; a.mask_src = mask_src;
  a.ld_out = g->ld_out; a.ld_res = ld_res; a.ld_mask = ld_mask; a.act = act;
  a.H = g->out_h; a.W = g->out_w;
  a.TH = (a.H + 1) / 2; a.TW = (a.W + 1) / 2;
  const long mtl = (long)g->n_img * a.TH * a.TW;
  {
    // the epilogue addresses out / residual / mask with 32-bit byte offsets below 2 GiB
    const long px = (long)g->n_img * a.H * a.W, lim = 1L << 29;
    if (px * g->ld_out >= lim || (residual && px * ld_res >= lim) ||
        (mask_src && px * ld_mask >= lim))
      return EMSA_E_SHAPE;
  }
  a.MT = (int)mtl;
  a.k_ch = g->k_ch; a.n_ch = g->n_ch;
  a.in_simg = (int)g->in_img_stride; a.in_srow = (int)g->in_row_stride; a.in_spx = g->in_px_stride;
  // 64-channel workgroups where the channels fill them; 32 otherwise (heads: 40, 96, 8 channels)
  const int nt = g->n_ch % 64 == 0 ? 2 : 1;
  const int wn = 32 * nt;
  a.tiles_m = (a.MT + kTiles - 1) / kTiles;
  a.tiles_n = (g->n_ch + wn - 1) / wn;
  a.ksteps = (g->k_ch + kK2 - 1) / kK2;
  a.in_bytes = (uint32_t)((size_t)g->n_img * g->in_img_stride * sizeof(float));
  a.u_bytes = (uint32_t)((size_t)16 * a.ksteps * kK2 * g->n_ch * sizeof(float));
  magic2((uint32_t)a.TW, a.mul_tw, a.sh_tw);
  magic2((uint32_t)a.TH, a.mul_th, a.sh_th);
  const size_t lds_main = (size_t)(16 * kTiles + 16 * wn) * kK2 * sizeof(float);
  const size_t lds_epi = (size_t)4 * kTiles * (wn + 4) * sizeof(float);
  const size_t lds = lds_main > lds_epi ? lds_main : lds_epi;
  // algorithmic = direct-convolution FLOPs (9 taps); the kernel executes 4/9 of them on the MFMA
  const double flops = 2.0 * g->n_img * a.H * a.W * (double)g->k_ch * g->n_ch * 9.0;
  const int ps = emsa_prof_begin(kProfClassWino3x3, flops, (hipStream_t)stream);
  if (nt == 2)
    hipLaunchKernelGGL((conv_wino2d_kernel<2>), dim3(a.tiles_m * a.tiles_n), dim3(256), lds,
                       (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((conv_wino2d_kernel<1>), dim3(a.tiles_m * a.tiles_n), dim3(256), lds,
                       (hipStream_t)stream, a);
  emsa_prof_end(ps, (hipStream_t)stream);
  return emsa_launch_status();
}
