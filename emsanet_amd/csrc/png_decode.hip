// PNG decoding on device: m complete PNG files, contiguous in one byte buffer with an offsets table
// (what csrc/png.hip leaves, and what a loader ships) -> the dense stack the stager and augmenter read.
// Foreign files: any deflate stream (stored / fixed / dynamic blocks, 32 KiB window), IDAT chunks split
// anywhere, ancillary chunks anywhere, filter types 0 ... 4.  Chunk CRC-32s are NOT verified (a flipped
// payload bit shows in the Adler-32 of the scanlines, which is).
//
// Two launches, no host step between them; the decode logic itself is csrc/png_inflate_core.h, which
// also builds as plain C++ (tools/png_decode_host.cpp) for the sanitizer runs on the CPU.
//   png_inflate_kernel    one wave per file -- files are the only parallelism a foreign deflate stream
//                         offers.  Chunk walk: signature, IHDR against the call, IDAT payloads joined
//                         into one zlib stream in the file's workspace slot (all lanes copy).  Inflate:
//                         wave-uniform symbol decoding out of LDS tables (rebuilt per dynamic block, the
//                         code lengths read serially, the tables filled by all lanes), the input held as
//                         one dword per lane so that a refill is a lane read; literals gathered 64 at a
//                         time, matches copied by all lanes.  Output: the filtered scanlines,
//                         h * (1 + stride) bytes in the slot; the last 32 KiB are mirrored in LDS, so
//                         that a match copy never waits for global memory.  Then the Adler-32, a
//                         partial sum per lane.  status[i] = EMSA_PNGD_*.
//   png_unfilter_kernel   one wave per file, a skewed pipeline: lane r owns row y0 + r of a band of 64
//                         rows and runs one pixel behind lane r - 1, so the pixel above arrives by lane
//                         shuffle, the one above left is the last step's, the one to the left the lane's
//                         own last result.  A band costs W + 63 steps for any mix of filter types.  The
//                         rows pass through LDS in tiles of 64 steps: coalesced loads in, the results
//                         overwrite the tile, coalesced stores out in the output layout (R,G,B or B,G,R;
//                         16-bit samples byte-swapped).  The band's last row stays in LDS for lane 0 of
//                         the next band.  A file with a non-zero status, or a filter type above 4, gets
//                         an all-zero image.
// Every loop ends on arbitrary bytes and nothing outside the file, its slot and its image is touched:
// see the header of png_inflate_core.h.  No atomics on global memory.
#include "common.h"

#define PNGD_DEVICE 1
#include "png_inflate_core.h"

namespace {

constexpr int kMaxSide = EMSA_PNG_MAX_SIDE;
constexpr int64_t kMaxFile = (int64_t)1 << 30;
constexpr int kSteps = 64;                  // pipeline steps per LDS tile

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
// bytes of a file's filtered scanlines, 256-aligned (the two halves of a slot share no cache line)
inline int64_t scan_bytes(int layout, int h, int w) {
  return align256((int64_t)h * (1 + (int64_t)w * pngd_bpp(layout)));
}
inline bool geometry_ok(int layout, int m, int h, int w) {
  return layout >= EMSA_PNG_GRAY8 && layout <= EMSA_PNG_GRAY16 && m >= 1 && m <= 65535 && h >= 1 &&
         h <= kMaxSide && w >= 1 && w <= kMaxSide;
}

// grid (m), 64 threads.  slot: [zcap bytes of zlib stream][scanlines]
__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ data,
                                                         const int64_t* __restrict__ offsets,
                                                         int64_t data_bytes, int layout, int H, int W,
                                                         uint8_t* ws, int64_t slot_bytes, uint32_t zcap,
                                                         int32_t* __restrict__ status) {
  __shared__ PngdTables tables;
  const int img = blockIdx.x;
  const int64_t o0 = offsets[img], o1 = offsets[img + 1];
  int st = EMSA_PNGD_CHUNK;
  if (o0 >= 0 && o1 >= o0 && o1 <= data_bytes && o1 - o0 <= kMaxFile) {
    uint8_t* z = ws + (int64_t)img * slot_bytes;
    uint8_t* scan = z + zcap;
    const uint32_t cap = (uint32_t)H * (1u + (uint32_t)W * (uint32_t)pngd_bpp(layout));
    uint32_t zlen = 0u;
    st = pngd_walk(data + o0, (uint32_t)(o1 - o0), layout, H, W, z, zcap, &zlen);
    __syncthreads();
    if (st == EMSA_PNGD_OK) st = pngd_inflate(z, zlen, scan, cap, tables);
  }
  if (threadIdx.x == 0) status[img] = st;
}

// grid (m), 64 threads
template <int BPP>
__global__ __launch_bounds__(64) void png_unfilter_kernel(const uint8_t* ws, int64_t slot_bytes,
                                                          uint32_t zcap, int H, int W, int mode,
                                                          uint8_t* __restrict__ dst, int32_t* status) {
  constexpr int kPitch = kSteps * BPP + 4;             // an odd number of dwords: lanes on distinct banks
  __shared__ uint8_t tile[64 * kPitch];
  __shared__ uint8_t uprow[kMaxSide * BPP];
  const int lane = threadIdx.x, img = blockIdx.x;
  const uint32_t stride = (uint32_t)W * BPP, rowlen = 1u + stride;
  const uint8_t* scan = ws + (int64_t)img * slot_bytes + zcap;
  uint8_t* out = dst + (size_t)img * H * stride;

  int st = status[img];
  if (st == EMSA_PNGD_OK) {
    bool bad = false;
    for (int y = lane; y < H; y += 64) bad = bad || scan[(size_t)y * rowlen] > 4u;
    if (__any(bad)) {
      st = EMSA_PNGD_FILTER;
      if (lane == 0) status[img] = st;
    }
  }
  if (st != EMSA_PNGD_OK) {
    const size_t total = (size_t)H * stride;
    for (size_t i = lane; i < total; i += 64) out[i] = 0;
    return;
  }

  for (uint32_t i = lane; i < stride; i += 64u) uprow[i] = 0;
  __syncthreads();
  for (int y0 = 0; y0 < H; y0 += 64) {
    const int rows = H - y0 < 64 ? H - y0 : 64;
    const bool live = lane < rows;
    const uint32_t f = live ? scan[(size_t)(y0 + lane) * rowlen] : 0u;
    uint32_t a = 0u, c = 0u;                           // packed pixels: byte k = sample byte k
    const int steps = W + rows - 1;
    for (int t0 = 0; t0 < steps; t0 += kSteps) {
      // tile row r = the bytes of pixels t0 - r ... t0 - r + 63 of row y0 + r
      // (the loads are unconditional, from a clamped place in the same row, so that several rows' are in
      // flight at once; only the LDS store is conditional)
#pragma unroll 8
      for (int r = 0; r < rows; ++r) {
        const uint8_t* src = scan + (size_t)(y0 + r) * rowlen + 1u;
        const int first = (t0 - r) * BPP;
#pragma unroll
        for (int j = 0; j < BPP; ++j) {
          const int col = lane + 64 * j, xb = first + col;
          const int xc = xb < 0 ? 0 : (xb < (int)stride ? xb : (int)stride - 1);
          const uint8_t v = src[xc];
          if (xb == xc) tile[r * kPitch + col] = v;
        }
      }
      __syncthreads();
      for (int s = 0; s < kSteps; ++s) {
        const int t = t0 + s, x = t - lane;
        uint32_t b = (uint32_t)__shfl_up((int)a, 1);
        if (lane == 0) {
          b = 0u;
          if (t < W) {
#pragma unroll
            for (int k = 0; k < BPP; ++k) b |= (uint32_t)uprow[t * BPP + k] << (8 * k);
          }
        }
        uint32_t o = 0u;
        if (live && x >= 0 && x < W) {
#pragma unroll
          for (int k = 0; k < BPP; ++k) {
            const uint32_t raw = tile[lane * kPitch + s * BPP + k];
            const uint32_t v = (raw + pngd_predict(f, (a >> (8 * k)) & 255u, (b >> (8 * k)) & 255u,
                                                   (c >> (8 * k)) & 255u)) & 255u;
            tile[lane * kPitch + s * BPP + k] = (uint8_t)v;
            if (lane == 63) uprow[x * BPP + k] = (uint8_t)v;   // (x = t - 63: behind lane 0's reads)
            o |= v << (8 * k);
          }
        }
        c = b;
        a = o;
      }
      __syncthreads();
      for (int r = 0; r < rows; ++r) {
        uint8_t* to = out + (size_t)(y0 + r) * stride;
        const int first = (t0 - r) * BPP;
#pragma unroll
        for (int j = 0; j < BPP; ++j) {
          const int col = lane + 64 * j, xb = first + col;
          if (xb >= 0 && xb < (int)stride) to[pngd_out_col(mode, (uint32_t)xb)] = tile[r * kPitch + col];
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" int64_t emsa_png_decode_ws_bytes(int32_t layout, int32_t m, int32_t h, int32_t w,
                                            int64_t file_bytes) {
  if (!geometry_ok(layout, m, h, w) || file_bytes < 1 || file_bytes > kMaxFile) return EMSA_E_SHAPE;
  return (int64_t)m * (align256(file_bytes) + scan_bytes(layout, h, w));
}

extern "C" int emsa_png_decode(const uint8_t* data, const int64_t* offsets, int64_t data_bytes, int32_t m,
                               int32_t layout, int32_t order, int32_t h, int32_t w, void* dst,
                               int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
  if (!geometry_ok(layout, m, h, w) || (order != EMSA_PNGD_RGB && order != EMSA_PNGD_BGR) || data_bytes < 0)
    return EMSA_E_SHAPE;
  const int64_t scan = scan_bytes(layout, h, w);
  const int64_t slot = (ws_bytes / m) & ~(int64_t)255;
  if (slot < scan + 256) return EMSA_E_SHAPE;
  if (!data || !offsets || !dst || !status || !ws) return EMSA_E_ARG;
  if ((uintptr_t)ws % 16 || (uintptr_t)offsets % 8 || (uintptr_t)status % 4) return EMSA_E_ARG;
  if (layout == EMSA_PNG_GRAY16 && (uintptr_t)dst % 2) return EMSA_E_ARG;
  const int64_t zcap64 = slot - scan;
  const uint32_t zcap = (uint32_t)(zcap64 < kMaxFile ? zcap64 : kMaxFile);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(png_inflate_kernel, dim3(m), dim3(64), 0, st, data, offsets, data_bytes, layout, h, w,
                     (uint8_t*)ws, slot, zcap, status);
  const int mode = pngd_store_mode(layout, order);
  if (layout == EMSA_PNG_GRAY8)
    hipLaunchKernelGGL(png_unfilter_kernel<1>, dim3(m), dim3(64), 0, st, (const uint8_t*)ws, slot, zcap, h, w,
                       mode, (uint8_t*)dst, status);
  else if (layout == EMSA_PNG_BGR8)
    hipLaunchKernelGGL(png_unfilter_kernel<3>, dim3(m), dim3(64), 0, st, (const uint8_t*)ws, slot, zcap, h, w,
                       mode, (uint8_t*)dst, status);
  else
    hipLaunchKernelGGL(png_unfilter_kernel<2>, dim3(m), dim3(64), 0, st, (const uint8_t*)ws, slot, zcap, h, w,
                       mode, (uint8_t*)dst, status);
  return emsa_launch_status();
}
