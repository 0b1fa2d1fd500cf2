// 2-D Winograd F(3x3,2x2) weight gradient on fp32 MFMA for the stride-1, "same"-padded dense 3x3
// convolutions (decoders, merged heads): the transpose of conv_wino2d.hip and the 2-D nesting of
// the F(3,2) row form in conv_mfma.hip (conv_wgrad1d_wino_kernel).
//
// Per 2x2 tile e of dy and its 4x4 input patch d (rows / columns 2t-1 .. 2t+2):
//   E = G' e G'^T        G' rows: (e0, e0+e1, e0-e1, -e1)
//   D = B^T d B          B^T rows: (d0-d2, d1+d2, d2-d1, d1-d3)
//   M_ij[co][ci] = sum_tiles E_ij[tile][co] * D_ij[tile][ci]          16 GEMMs, K = tiles = pixels / 4
//   dW = A'^T M A'       per direction: dW_0 = M0+(M1+M2)/2, dW_1 = (M1-M2)/2, dW_2 = (M1+M2)/2+M3
// 16 of the 36 direct multiplies per tile (the row form runs 24) and every operand staged ONCE (the
// row form stages dy and x once per kernel row).  Coefficients 1 and 1/2: exact in fp32.
//
// Workgroup = 32 cout x 64 cin, 4 waves: wave j owns column component j and all four row
// components (8 accumulator tiles of 32x32 = 128 registers, two workgroups per CU).  K step = 8
// tiles.  The loaders apply the ROW direction of both transforms once per element on the way to LDS
// (a d thread holds the four patch rows of one (tile, patch column, float4), an e thread the two
// rows of one (tile, column, float4)), staged [row comp][column][tile][channel]: lanes run along
// the channels, the conflict-free scalar reads of the row kernel.  The COLUMN direction stays in
// the consuming wave: operand = a + sg * b of two LDS reads.  A wave loads the tiles (wave, wave +
// 4) of a step, so the tile -> (image, line, column) decomposition is scalar work; rows above /
// below the image, columns past a line end, the virtual row / column of an odd size, tiles past
// the last one and channels past the tensor's read zero through out-of-range buffer offsets: no
// masks, no branch around a load.  -e1 is staged as +e1 (row AND column direction); the signs are
// folded into the output transform.
// Split-K over contiguous tile ranges, work items in XCD-contiguous order; a workgroup applies
// A'^T . A' to its accumulators (row direction in registers, column direction through LDS) and
// stores 9 partial tiles [tap][32][64] with coalesced 16-byte stores; wgrad_wino2d_reduce_kernel
// sums the splits in a fixed order into the OIHW parameter layout or the packed [tap][cout][cin]
// form.  No atomics, no zero fill: bit-reproducible.  The bias gradient (column sums of dy) is
// summed by the e loaders of the workgroups of cin tile 0.
#include "common.h"
#include "prof.h"

namespace {

constexpr int kTK = 8;             // 2x2 tiles per K step
constexpr int kBCO = 32, kBCI = 64;
constexpr int kTileF = 9 * kBCO * kBCI;   // floats of one workgroup's partial result
constexpr uint32_t kOOBg = 0x80000000u;

typedef float vf32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t grsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 gbuf_ld4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}
__device__ __forceinline__ uint32_t gdiv(uint32_t n, uint32_t mul, uint32_t sh) {
  return (__umulhi(n, mul) + n) >> sh;
}
__device__ __forceinline__ float4 gsub4(float4 a, float4 b) {
  const vf32x2 lo = vf32x2{a.x, a.y} - vf32x2{b.x, b.y}, hi = vf32x2{a.z, a.w} - vf32x2{b.z, b.w};
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ float4 gadd4(float4 a, float4 b) {
  const vf32x2 lo = vf32x2{a.x, a.y} + vf32x2{b.x, b.y}, hi = vf32x2{a.z, a.w} + vf32x2{b.z, b.w};
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}

struct Wgrad2dArgs {
  const float* in;
  const float* dout;
  float* ws;                        // [split][tile][9 taps][32 co][64 ci]
  float* ws_bias;                   // [split][co tile][32], or NULL
  int H, W, TH, TW, MT;             // image size, tiles per column / line, total tiles
  int n_ch, k_ch;                   // cout, cin
  int in_simg, in_srow, in_spx;     // element strides of x
  int ld_dy;                        // pixel stride of dy
  int steps_total, steps_per_split, n_ci_tiles, n_co_tiles, n_tiles;
  uint32_t in_bytes, dy_bytes;
  uint32_t mul_tw, sh_tw, mul_th, sh_th;   // magic division by TW and by TH
};

__global__ __launch_bounds__(256, 2) void conv_wgrad_wino2d_kernel(const Wgrad2dArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const Es = smem;                          // [4 i][2 col][kTK][kBCO]
  float* const Ds = smem + 4 * 2 * kTK * kBCO;     // [4 i][4 col][kTK][kBCI]
  constexpr int EI = 2 * kTK * kBCO, DI = 4 * kTK * kBCI;   // row-component strides

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  // work item = split * n_tiles + tile: an XCD (own L2) gets all the tiles of a few tile ranges
  const int wg = emsa_xcd_remap(blockIdx.x, gridDim.x);
  const int tile = wg % p.n_tiles, ks = wg / p.n_tiles;
  const int ci_t = tile % p.n_ci_tiles, co_t = tile / p.n_ci_tiles;
  const int co0 = co_t * kBCO, ci0 = ci_t * kBCI;
  const int s_begin = ks * p.steps_per_split;
  const int s_end = min(s_begin + p.steps_per_split, p.steps_total);
  const __amdgpu_buffer_rsrc_t rs_in = grsrc(p.in, p.in_bytes);
  const __amdgpu_buffer_rsrc_t rs_dy = grsrc(p.dout, p.dy_bytes);

  // ---- loader lanes --------------------------------------------------------------------------
  // d: lane = (patch column, float4 of the 64 cin); the wave's two tiles are wave, wave + 4
  const int dc4 = (lane & 15) * 4, dcol = lane >> 4;
  const bool dchok = ci0 + dc4 < p.k_ch;
  const int d_lanec = (dcol * p.in_spx + ci0 + dc4) * 4;      // bytes from pixel (y, 2 tx - 1)
  // e: lanes 0..31 = (tile of the two, column, float4 of the 32 cout)
  const int ec4 = (lane & 7) * 4, ecol = (lane >> 3) & 1, et2 = (lane >> 4) & 1;
  const bool elane = lane < 32;
  const bool echok = elane && co0 + ec4 < p.n_ch;
  const int e_lanec = (ecol * p.ld_dy + co0 + ec4) * 4;       // bytes from pixel (2 ty, 2 tx)
  const int dy_row = p.W * p.ld_dy * 4;

  float4 rd[2][4], re[2];
  float4 bsum = emsa_zero4();
  auto load_regs = [&](int s) {
    uint32_t e_base[2];
    bool e_xok[2], e_r1ok[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      // wave-uniform: the tile's position is scalar work
      const int q = s * kTK + wave + 4 * t2;
      const bool qok = q < p.MT;
      const uint32_t qq = qok ? (uint32_t)q : 0u;
      const int line = (int)gdiv(qq, p.mul_tw, p.sh_tw);               // img * TH + ty
      const int tx = (int)qq - line * p.TW;
      const int img = (int)gdiv((uint32_t)line, p.mul_th, p.sh_th);
      const int ty = line - img * p.TH;
      const int y0 = 2 * ty, x0 = 2 * tx;
      const int x = x0 - 1 + dcol;
      const bool cok = qok && dchok && x >= 0 && x < p.W;
      // (negative for the first tile of the tensor; an in-range element's sum is not)
      const int sb = (img * p.in_simg + (y0 - 1) * p.in_srow + (x0 - 1) * p.in_spx) * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int y = y0 - 1 + r;
        const bool ok = cok && y >= 0 && y < p.H;
        rd[t2][r] = gbuf_ld4(rs_in, ok ? (uint32_t)(sb + r * p.in_srow * 4 + d_lanec) : kOOBg);
      }
      e_base[t2] = (uint32_t)(((img * p.H + y0) * p.W + x0) * p.ld_dy * 4);
      e_xok[t2] = qok && x0 + ecol < p.W;
      e_r1ok[t2] = y0 + 1 < p.H;
    }
    const uint32_t eb = (et2 ? e_base[1] : e_base[0]) + (uint32_t)e_lanec;
    const bool ok0 = echok && (et2 ? e_xok[1] : e_xok[0]);
    const bool ok1 = ok0 && (et2 ? e_r1ok[1] : e_r1ok[0]);
    re[0] = gbuf_ld4(rs_dy, ok0 ? eb : kOOBg);
    re[1] = gbuf_ld4(rs_dy, ok1 ? eb + (uint32_t)dy_row : kOOBg);
  };
  auto store_lds = [&]() {
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      float* const d = Ds + (dcol * kTK + wave + 4 * t2) * kBCI + dc4;
      emsa_st4(d + 0 * DI, gsub4(rd[t2][0], rd[t2][2]));
      emsa_st4(d + 1 * DI, gadd4(rd[t2][1], rd[t2][2]));
      emsa_st4(d + 2 * DI, gsub4(rd[t2][2], rd[t2][1]));
      emsa_st4(d + 3 * DI, gsub4(rd[t2][1], rd[t2][3]));
    }
    if (elane) {
      float* const e = Es + (ecol * kTK + wave + 4 * et2) * kBCO + ec4;
      const float4 es = gadd4(re[0], re[1]);
      bsum = gadd4(bsum, es);                      // bias gradient = column sums of dy
      emsa_st4(e + 0 * EI, re[0]);
      emsa_st4(e + 1 * EI, es);
      emsa_st4(e + 2 * EI, gsub4(re[0], re[1]));
      emsa_st4(e + 3 * EI, re[1]);                 // -e1 staged as +e1
    }
  };

  // wave j: E_ij = Es[i][ea] + sge * Es[i][eb] (e0, e0+e1, e0-e1, +e1: sge = 0 keeps one column),
  //         D_ij = Ds[i][ca] + sgd * Ds[i][cb]
  const int ea = wave == 3 ? 1 : 0, eb_ = wave == 0 ? 0 : 1;
  const float sge = wave == 1 ? 1.f : wave == 2 ? -1.f : 0.f;
  const int ca = wave == 0 ? 0 : wave == 2 ? 2 : 1;
  const int cb = wave == 2 ? 1 : wave == 3 ? 3 : 2;
  const float sgd = wave == 1 ? 1.f : -1.f;
  const vf32x2 sgd2 = {sgd, sgd};

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][h][r] = 0.f;

  if (s_begin < s_end) {
    load_regs(s_begin);
    store_lds();
  }
  __syncthreads();

  const float* const e0 = Es + (ea * kTK + lh) * kBCO + l31;
  const float* const e1 = Es + (eb_ * kTK + lh) * kBCO + l31;
  const float* const d0 = Ds + (ca * kTK + lh) * kBCI + l31;
  const float* const d1 = Ds + (cb * kTK + lh) * kBCI + l31;
  for (int s = s_begin; s < s_end; ++s) {
    const bool has_next = s + 1 < s_end;
    __builtin_amdgcn_s_setprio(3);           // the next step's loads go out first
    if (has_next) load_regs(s + 1);
    __builtin_amdgcn_s_setprio(1);
    // K index of the MFMA = tile: lane half lh takes tile 2 * kk + lh of the step's 8.
    // (tried: the LDS reads two (kk, i) units ahead with the order pinned by sched_group_barrier
    //  -- 3 % slower than the compiler's own order; the next-but-one step's loads issued right
    //  behind store_lds instead of here -- no faster: DESIGN.md 4.2)
#pragma unroll
    for (int kk = 0; kk < kTK / 2; ++kk) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int eo = i * EI + kk * 2 * kBCO, dofs = i * DI + kk * 2 * kBCI;
        const float ev = __builtin_fmaf(e1[eo], sge, e0[eo]);
        const vf32x2 dv = __builtin_elementwise_fma(vf32x2{d1[dofs], d1[dofs + 32]}, sgd2,
                                                    vf32x2{d0[dofs], d0[dofs + 32]});
        acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ev, dv.x, acc[i][0], 0, 0, 0);
        acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ev, dv.y, acc[i][1], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    if (has_next) store_lds();
    __syncthreads();
  }

  // ---- output transform -----------------------------------------------------------------------
  // row direction in registers (M_3j was accumulated with +e1, i.e. negated):
  //   R_0 = M0 + (M1+M2)/2    R_1 = (M1-M2)/2    R_2 = (M1+M2)/2 - M3'
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float m0 = acc[0][h][r], m1 = acc[1][h][r], m2 = acc[2][h][r], m3 = acc[3][h][r];
      const float hs = 0.5f * (m1 + m2);
      acc[0][h][r] = m0 + hs;
      acc[1][h][r] = 0.5f * (m1 - m2);
      acc[2][h][r] = hs - m3;
    }
  // column direction through LDS, one kernel row k at a time: the four waves stage R_k of their
  // column component as [j][32 co][64 ci]; thread (row = tid / 16 + 16 u, float4 = tid % 16)
  // forms the three taps of kernel row k (wave 3's component is negated, as above) and stores them
  float* const stage = smem;
  float* const wt = p.ws + ((size_t)ks * p.n_tiles + tile) * kTileF;
  const int oc4 = (tid & 15) * 4, orow = tid >> 4;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    __syncthreads();                     // the K loop's buffers / the previous row are consumed
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
        stage[(wave * kBCO + row) * kBCI + h * 32 + l31] = acc[k][h][r];
      }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = orow + 16 * u;
      const float4 r0 = emsa_ld4(stage + (0 * kBCO + row) * kBCI + oc4);
      const float4 r1 = emsa_ld4(stage + (1 * kBCO + row) * kBCI + oc4);
      const float4 r2 = emsa_ld4(stage + (2 * kBCO + row) * kBCI + oc4);
      const float4 r3 = emsa_ld4(stage + (3 * kBCO + row) * kBCI + oc4);
      const float4 s12 = gadd4(r1, r2), d12 = gsub4(r1, r2);
      const float4 hs = make_float4(0.5f * s12.x, 0.5f * s12.y, 0.5f * s12.z, 0.5f * s12.w);
      emsa_st4(wt + ((k * 3 + 0) * kBCO + row) * kBCI + oc4, gadd4(r0, hs));
      emsa_st4(wt + ((k * 3 + 1) * kBCO + row) * kBCI + oc4,
               make_float4(0.5f * d12.x, 0.5f * d12.y, 0.5f * d12.z, 0.5f * d12.w));
      emsa_st4(wt + ((k * 3 + 2) * kBCO + row) * kBCI + oc4, gsub4(hs, r3));
    }
  }

  if (p.ws_bias != nullptr && ci_t == 0) {
    float* const red = smem;             // [16: wave, tile of the two, column][kBCO]
    __syncthreads();                     // everyone has read `stage`
    if (elane) emsa_st4(red + (wave * 4 + et2 * 2 + ecol) * kBCO + ec4, bsum);
    __syncthreads();
    if (tid < kBCO) {
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) a += red[r * kBCO + tid];
      p.ws_bias[((size_t)ks * p.n_co_tiles + co_t) * kBCO + tid] = a;
    }
  }
}

// Sum over the splits of ws[split][tile][tap][co_l][ci_l] in a fixed order; dbias[co] = sum of
// ws_bias[split][co tile][co_l].  A workgroup = 16 float4 columns x 16 slots; the slots are G split
// groups x 16 / G rows (row = (tile, tap, co_l)): many splits and few tiles (the heads at /4) give
// a row to 16 groups, few splits and many tiles (512 channels) give every thread a row of its own.
// Eight independent loads in flight per thread.  The workgroups behind the weight rows reduce the
// bias.  packed = 0: OIHW [co][ci][3][3]; 1: [tap][cout][cin].
__global__ __launch_bounds__(256) void wgrad_wino2d_reduce_kernel(
    const float* __restrict__ ws, const float* __restrict__ ws_bias, int splits, int n_tiles,
    int n_ci_tiles, int n_co_tiles, int n_ch, int k_ch, float* __restrict__ dw,
    float* __restrict__ dbias, int packed, int G, int weight_blocks) {
  __shared__ float4 red[16][16];
  __shared__ float redb[8][kBCO];
  const int tid = threadIdx.x, bid = blockIdx.x;
  if (bid < weight_blocks) {
    const int col = tid & 15, slot = tid >> 4;
    const int g = slot % G, rw = slot / G;
    const long rowi = (long)bid * (16 / G) + rw;
    const bool valid = rowi < (long)n_tiles * 9 * kBCO;
    const int tl = (int)(rowi / (9 * kBCO)), rem = (int)(rowi % (9 * kBCO));
    const int tap = rem / kBCO, co_l = rem % kBCO;
    const float* src = ws + (size_t)tl * kTileF + (tap * kBCO + co_l) * kBCI + col * 4;
    const size_t sstride = (size_t)n_tiles * kTileF;
    float4 a = emsa_zero4();
    const int nsp = valid ? splits : 0;
    for (int sp = g; sp < nsp; sp += 8 * G) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = sp + u * G < nsp ? emsa_ld4(src + (size_t)(sp + u * G) * sstride) : emsa_zero4();
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w;
      }
    }
    red[slot][col] = a;
    __syncthreads();
    if (g == 0 && valid) {
      for (int k = 1; k < G; ++k) {
        const float4 v = red[slot + k][col];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      }
      const int co = (tl / n_ci_tiles) * kBCO + co_l;
      const int ci = (tl % n_ci_tiles) * kBCI + col * 4;
      if (co < n_ch && ci < k_ch) {               // k_ch is a multiple of 4
        if (packed) {
          emsa_st4(dw + ((size_t)tap * n_ch + co) * k_ch + ci, a);
        } else {
          float* o = dw + ((size_t)co * k_ch + ci) * 9 + tap;
          o[0] = a.x; o[9] = a.y; o[18] = a.z; o[27] = a.w;
        }
      }
    }
  } else if (dbias != nullptr) {
    const int co_t = bid - weight_blocks;
    const int c = tid & 31, g = tid >> 5;
    float a = 0.f;
    for (int sp = g; sp < splits; sp += 32) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        v[u] = sp + 8 * u < splits ? ws_bias[((size_t)(sp + 8 * u) * n_co_tiles + co_t) * kBCO + c] : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) a += v[u];
    }
    redb[g][c] = a;
    __syncthreads();
    if (g == 0) {
#pragma unroll
      for (int k = 1; k < 8; ++k) a += redb[k][c];
      const int co = co_t * kBCO + c;
      if (co < n_ch) dbias[co] = a;
    }
  }
}

inline void gmagic2(uint32_t d, uint32_t& mul, uint32_t& sh) {
  uint32_t s = 0;
  while ((1ull << s) < d) ++s;
  sh = s;
  mul = (uint32_t)(((1ull << 32) * ((1ull << s) - d)) / d + 1);
}

struct Wgrad2dPlan {
  Wgrad2dArgs a;
  int ksplit;
};

bool geom_wgrad2d(int32_t dtype, const EmsaConvGeom* g) {
  if (!g || dtype != EMSA_DT_F32) return false;
  if (g->out_pix_img || g->out_pix_row || g->out_pix_px || g->out_pix_off) return false;
  if (!(g->kh == 3 && g->kw == 3 && g->off_h == -1 && g->off_w == -1 && g->step_h == 1 &&
        g->step_w == 1))
    return false;
  if (g->mul_h != 1 || g->mul_w != 1 || g->div_h != 1 || g->div_w != 1) return false;
  if (g->n_img < 1 || g->in_h < 1 || g->in_w < 1 || g->k_ch < 4 || g->n_ch < 4) return false;
  if (g->in_h != g->out_h || g->in_w != g->out_w) return false;
  if ((g->k_ch & 3) || (g->n_ch & 3) || (g->ld_out & 3) || (g->in_px_stride & 3) ||
      (g->in_row_stride & 3) || (g->in_img_stride & 3))
    return false;
  if (g->ld_out < g->n_ch || g->in_px_stride < g->k_ch) return false;
  // 32-bit byte offsets below 2 GiB into both tensors
  const long lim = 1L << 29;
  if ((long)g->n_img * g->in_img_stride >= lim) return false;
  if ((long)(g->in_h + 2) * g->in_row_stride >= lim) return false;
  if ((long)g->n_img * g->out_h * g->out_w * g->ld_out >= lim) return false;
  return true;
}

bool plan_wgrad2d(int32_t dtype, const EmsaConvGeom* g, Wgrad2dPlan& pl) {
  if (!geom_wgrad2d(dtype, g)) return false;
  Wgrad2dArgs& a = pl.a;
  a.H = g->out_h; a.W = g->out_w;
  a.TH = (a.H + 1) / 2; a.TW = (a.W + 1) / 2;
  a.MT = (int)((long)g->n_img * a.TH * a.TW);
  a.n_ch = g->n_ch; a.k_ch = g->k_ch;
  a.in_simg = (int)g->in_img_stride; a.in_srow = (int)g->in_row_stride; a.in_spx = g->in_px_stride;
  a.ld_dy = g->ld_out;
  a.n_co_tiles = (g->n_ch + kBCO - 1) / kBCO;
  a.n_ci_tiles = (g->k_ch + kBCI - 1) / kBCI;
  a.n_tiles = a.n_co_tiles * a.n_ci_tiles;
  a.steps_total = (a.MT + kTK - 1) / kTK;
  a.in_bytes = (uint32_t)((size_t)g->n_img * g->in_img_stride * sizeof(float));
  a.dy_bytes = (uint32_t)((size_t)g->n_img * a.H * a.W * g->ld_out * sizeof(float));
  gmagic2((uint32_t)a.TW, a.mul_tw, a.sh_tw);
  gmagic2((uint32_t)a.TH, a.mul_th, a.sh_th);
  // split-K: one round of resident workgroups (2 per CU); a split is at least 8 K steps (256
  // pixels) -- EMSA_WGRAD2D_BLOCKS: tuning only
  static const int forced_blocks = [] {
    const char* e = getenv("EMSA_WGRAD2D_BLOCKS");
    return e ? atoi(e) : 0;
  }();
  const int target_blocks = forced_blocks > 0 ? forced_blocks : 512;
  int ksplit = target_blocks / a.n_tiles;
  const int max_split = (a.steps_total + 7) / 8;
  if (ksplit > max_split) ksplit = max_split;
  if (ksplit < 1) ksplit = 1;
  a.steps_per_split = (a.steps_total + ksplit - 1) / ksplit;
  pl.ksplit = (a.steps_total + a.steps_per_split - 1) / a.steps_per_split;
  return true;
}

}  // namespace

// 1 if the weight gradient of `g` (forward geometry of the conv, activations of `dtype`) is a
// dense stride-1 3x3 "same" fp32 conv on tensors the kernel's 32-bit offsets reach
extern "C" int emsa_conv_wgrad_wino2d_supported(int32_t dtype, const EmsaConvGeom* g) {
  return geom_wgrad2d(dtype, g) ? 1 : 0;
}

extern "C" int64_t emsa_conv_wgrad_wino2d_ws_bytes(int32_t dtype, const EmsaConvGeom* g) {
  Wgrad2dPlan pl;
  if (!plan_wgrad2d(dtype, g, pl)) return 0;
  return (int64_t)pl.ksplit * ((int64_t)pl.a.n_tiles * kTileF + (int64_t)pl.a.n_co_tiles * kBCO) *
         (int64_t)sizeof(float);
}

// K steps per split of the plan (tests place a tile count next to a split boundary with it)
extern "C" int emsa_conv_wgrad_wino2d_split_steps(int32_t dtype, const EmsaConvGeom* g) {
  Wgrad2dPlan pl;
  if (!plan_wgrad2d(dtype, g, pl)) return EMSA_E_SHAPE;
  return pl.a.steps_per_split;
}

extern "C" int emsa_conv_wgrad_wino2d(int32_t dtype, const EmsaConvGeom* g, const void* in,
                                      const void* dout, float* dw, float* dbias, float* ws,
                                      int32_t packed, void* stream) {
  Wgrad2dPlan pl;
  if (!plan_wgrad2d(dtype, g, pl)) return EMSA_E_SHAPE;
  if (!in || !dout || !dw || !ws) return EMSA_E_ARG;
  auto al16 = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  if (!al16(in) || !al16(dout) || !al16(dw) || !al16(ws)) return EMSA_E_SHAPE;
  Wgrad2dArgs& a = pl.a;
  a.in = (const float*)in; a.dout = (const float*)dout;
  a.ws = ws;
  a.ws_bias = dbias ? ws + (size_t)pl.ksplit * a.n_tiles * kTileF : nullptr;
  hipStream_t st = (hipStream_t)stream;
  constexpr size_t lds = (size_t)(4 * 2 * kTK * kBCO + 4 * 4 * kTK * kBCI) * sizeof(float);
  static_assert(lds >= (size_t)4 * kBCO * kBCI * sizeof(float), "the epilogue stage overlays the K loop's buffers");
  // algorithmic = direct-convolution FLOPs (9 taps); bytes: x and dy read once, dw written once
  const double px = (double)g->n_img * a.H * a.W;
  const double flops = 2.0 * px * (double)g->k_ch * g->n_ch * 9.0;
  const double bytes = px * (g->k_ch + g->n_ch) * 4.0 + 9.0 * g->n_ch * g->k_ch * 4.0;
  const int ps = emsa_prof_begin(kProfClassWgrad3x3, flops, st, bytes);
  hipLaunchKernelGGL(conv_wgrad_wino2d_kernel, dim3(a.n_tiles * pl.ksplit), dim3(256), lds, st, a);
  // split groups of the reduction: at most 8 splits per thread
  int G = 1;
  while (G < 16 && pl.ksplit > 8 * G) G *= 2;
  const long rows = (long)a.n_tiles * 9 * kBCO;
  const int rpb = 16 / G;
  const int weight_blocks = (int)((rows + rpb - 1) / rpb);
  hipLaunchKernelGGL(wgrad_wino2d_reduce_kernel, dim3(weight_blocks + (dbias ? a.n_co_tiles : 0)),
                     dim3(256), 0, st, ws, a.ws_bias, pl.ksplit, a.n_tiles, a.n_ci_tiles,
                     a.n_co_tiles, a.n_ch, a.k_ch, dw, dbias, packed ? 1 : 0, G, weight_blocks);
  emsa_prof_end(ps, st);
  return emsa_launch_status();
}
