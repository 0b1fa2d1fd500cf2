// PNG encoding on device: a stack of dense uint8 / uint16 images (the outputs of csrc/export.hip) ->
// one complete, standalone PNG file per image, contiguous in one byte buffer, with an offsets table.
// Everything is made here, both checksums included; the host never touches a pixel or stream byte.
//
// File: signature, IHDR, one IDAT chunk per strip of kRows rows, IEND.  The IDAT payloads form ONE zlib
// stream: `78 01`, then per strip one fixed-Huffman block (BTYPE=01) closed by an empty stored block
// (the "sync flush" 00 00 FF FF, which ends the strip on a byte boundary), behind the last strip an
// empty stored block with BFINAL=1, then the big-endian Adler-32 of the filtered scanlines.
// Filter type 0 on every row.  Tokens: literals, and matches of length 3 ... 258 at distance bpp
// (a run of equal pixels); the distance codes 0 ... 2 carry no extra bits.
//
// Three launches, no host step between them:
//   png_strip_kernel     one wave per strip.  The strip's filtered bytes (filter byte, samples in file
//                        order: R,G,B from B,G,R; big-endian 16-bit) are walked in tiles of 64, one byte
//                        per lane.  A lane continues a run when its byte equals the one bpp before it
//                        (shuffle; the last tile's bytes stay in a register); ballot gives the run
//                        structure of the tile.  Runs inside the tile are emitted by the lane at their
//                        start; the run open at the tile's end is carried (a count) into the next tile
//                        and emitted there by the wave as a whole, in chunks of 258.  A wave prefix sum
//                        over the token bit counts places every token; the bits are OR-ed into LDS and
//                        leave as whole dwords into the strip's own worst-case-sized slot.  The strip
//                        also leaves its byte count and its two Adler sums, the second already weighted
//                        for the strip's place in the image:  s1 = sum f[i],  s2 = sum (N - i) f[i]
//                        (i: index in the image's scanline stream of N bytes), both mod 65521 -- so that
//                        A = 1 + sum s1, B = N + sum s2 need no ordered combination.
//   png_layout_kernel    one workgroup per image: file start = sizes of the files before it, chunk
//                        position of every strip (scan of the strip sizes), Adler-32, signature, IHDR,
//                        IEND, offsets[].
//   png_assemble_kernel  one wave per strip: chunk length, type, the slot's bytes, CRC-32 (per chunk:
//                        no CRC combination), zlib header in the first chunk, Adler-32 in the last.
// Output bytes are a pure function of the input: no atomics on global memory, no order dependence.
#include "common.h"

namespace {

constexpr int kRows = 4;                    // rows per strip
constexpr int kMaxSide = EMSA_PNG_MAX_SIDE;
constexpr uint32_t kAdler = 65521u;
constexpr int kBitWords = 32;               // LDS dwords of a tile's bits: 31 pending + 3 x 18 (carried
                                            // run) + 64 x 9 (literals) = 661 bits = 21 dwords

inline int bpp_of(int layout) { return layout == EMSA_PNG_BGR8 ? 3 : (layout == EMSA_PNG_GRAY16 ? 2 : 1); }

// most bytes of deflate data a strip of n filtered bytes can make: 3 header bits, 9 bits per byte
// (a literal >= 144; a match never costs more than the literals it replaces), 7 bits end-of-block,
// 3 bits stored-block header, padding, LEN / NLEN; behind the last strip one more byte-aligned empty
// stored block
inline int64_t strip_bound(int64_t n, bool last) { return (9 * n + 13 + 7) / 8 + 4 + (last ? 5 : 0); }

struct Geo {
  int bpp, strips;
  int64_t rowlen, n_full, n_last, slot_bytes, bound;
};
inline Geo geometry(int layout, int h, int w) {
  Geo g;
  g.bpp = bpp_of(layout);
  g.strips = (h + kRows - 1) / kRows;
  g.rowlen = 1 + (int64_t)w * g.bpp;
  g.n_full = kRows * g.rowlen;
  g.n_last = (h - (g.strips - 1) * kRows) * g.rowlen;
  g.slot_bytes = (strip_bound(g.n_full, true) + 4 + 15) & ~(int64_t)15;     // whole-dword stores
  // signature 8, IHDR 25, IEND 12, zlib header 2, Adler-32 4; 12 bytes of framing per IDAT chunk
  g.bound = 51 + 12 * (int64_t)g.strips + (g.strips - 1) * strip_bound(g.n_full, false) +
            strip_bound(g.n_last, true);
  return g;
}

struct Ws {
  int64_t rec, dst, adler, slots, total;
};
inline Ws workspace(const Geo& g, int m) {
  const int64_t ns = (int64_t)m * g.strips;
  Ws s;
  s.rec = 0;                                          // uint4 per strip: bytes, s1, s2, -
  s.dst = s.rec + ns * 16;                            // int64 per strip: where its chunk starts
  s.adler = s.dst + ns * 8;                           // uint32 per image
  s.slots = (s.adler + (int64_t)m * 4 + 15) & ~(int64_t)15;
  s.total = s.slots + ns * g.slot_bytes;
  return s;
}

// ---- tokens ---------------------------------------------------------------------------------------
// (value, bit count), LSB first as deflate packs them; Huffman codes enter bit-reversed
__device__ __forceinline__ void literal_token(uint32_t v, uint32_t& val, uint32_t& nb) {
  const bool wide = v >= 144u;
  nb = wide ? 9u : 8u;
  val = __brev(wide ? 0x190u + (v - 144u) : 0x30u + v) >> (32u - nb);
}
// L in [3, 258]; drev: the 5-bit distance code, reversed
__device__ __forceinline__ void match_token(uint32_t L, uint32_t drev, uint32_t& val, uint32_t& nb) {
  uint32_t sym, e = 0u, extra = 0u;
  if (L <= 10u) sym = 254u + L;
  else if (L == 258u) sym = 285u;
  else {
    const uint32_t x = L - 3u;                          // 8 ... 254
    e = 29u - (uint32_t)__clz((int)x);                  // extra bits 1 ... 5
    sym = 261u + 4u * e + ((x >> e) & 3u);
    extra = x & ((1u << e) - 1u);
  }
  const uint32_t cb = sym < 280u ? 7u : 8u;
  const uint32_t code = sym < 280u ? sym - 256u : 0xC0u + (sym - 280u);
  val = (__brev(code) >> (32u - cb)) | (extra << cb) | (drev << (cb + e));
  nb = cb + e + 5u;
}

__device__ __forceinline__ void put_bits(uint32_t* bits, uint32_t pos, uint32_t val, uint32_t nb) {
  if (nb == 0u) return;
  const uint32_t w = pos >> 5, sh = pos & 31u;
  const uint64_t t = (uint64_t)val << sh;
  if (w < (uint32_t)kBitWords) atomicOr(&bits[w], (uint32_t)t);
  if ((uint32_t)(t >> 32) && w + 1u < (uint32_t)kBitWords) atomicOr(&bits[w + 1u], (uint32_t)(t >> 32));
}

// filtered byte p of a strip: rows of rowlen = 1 + rowbytes; the filter byte is 0
template <int BPP>
__device__ __forceinline__ uint32_t filtered_byte(const uint8_t* __restrict__ base, uint32_t p,
                                                  uint32_t rowlen) {
  const uint32_t r = p / rowlen, c = p - r * rowlen;
  if (c == 0u) return 0u;
  uint32_t j = c - 1u;
  if (BPP == 2) j ^= 1u;                                               // big-endian samples
  if (BPP == 3) { const uint32_t px = j / 3u; j = 6u * px + 2u - j; }  // 3 px + (2 - (j - 3 px))
  return base[(size_t)r * (rowlen - 1u) + j];
}

// grid (strips, m), 64 threads
template <int BPP>
__global__ __launch_bounds__(64) void png_strip_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                       int strips, uint32_t slot_bytes,
                                                       uint4* __restrict__ rec,
                                                       uint8_t* __restrict__ slots) {
  __shared__ uint32_t bits[kBitWords];
  const uint32_t lane = threadIdx.x;
  const int s = blockIdx.x, img = blockIdx.y;
  const uint32_t rowlen = 1u + (uint32_t)W * BPP;
  const int row0 = s * kRows;
  const int rows = H - row0 < kRows ? H - row0 : kRows;
  const uint32_t n = (uint32_t)rows * rowlen;                      // <= 4 * 12289
  const uint32_t N = (uint32_t)H * rowlen, P0 = (uint32_t)row0 * rowlen;   // <= 4096 * 12289
  const uint8_t* base = src + ((size_t)img * H + row0) * (rowlen - 1u);
  const size_t slot = (size_t)img * strips + s;
  uint32_t* out = reinterpret_cast<uint32_t*>(slots + slot * slot_bytes);
  const uint32_t slot_words = slot_bytes >> 2;
  constexpr uint32_t kDrev = BPP == 1 ? 0u : (BPP == 2 ? 16u : 8u);   // distance codes 0, 1, 2 reversed

  if (lane < (uint32_t)kBitWords) bits[lane] = lane == 0u ? 2u : 0u;   // BFINAL = 0, BTYPE = 01
  __syncthreads();
  uint32_t wpos = 0u, r = 3u;          // dwords stored; bits pending in bits[]
  uint32_t carry = 0u;                 // bytes of the run open at the end of the last tile, not yet emitted
  uint32_t prevv = 0u;                 // this lane's byte of the last tile
  uint32_t s1 = 0u, s2 = 0u;
  uint32_t vnext = lane < n ? filtered_byte<BPP>(base, lane, rowlen) : 0u;

  // one more tile than the bytes need when n is a multiple of 64: it closes the carried run
  for (uint32_t t0 = 0u; t0 <= n; t0 += 64u) {
    const uint32_t p = t0 + lane;
    const bool valid = p < n;
    const uint32_t v = vnext;
    vnext = p + 64u < n ? filtered_byte<BPP>(base, p + 64u, rowlen) : 0u;
    if (valid) {
      s1 += v;
      s2 = (s2 + v * ((N - P0 - p) % kAdler)) % kAdler;
    }
    const int from = (int)((lane - (uint32_t)BPP) & 63u);
    const uint32_t a = (uint32_t)__shfl((int)v, from), b = (uint32_t)__shfl((int)prevv, from);
    const uint32_t before = lane >= (uint32_t)BPP ? a : b;
    const bool eq = valid && p >= (uint32_t)BPP && v == before;
    const uint64_t m = __ballot(eq);
    const uint32_t lead = m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);   // lanes continuing the carry

    // the carried run, by the wave as a whole (the values below are the same in every lane):
    // token k is kept by lane k
    uint32_t cval = 0u, cnb = 0u, cpos = 0u, cbits = 0u, cn = 0u;
    uint32_t pend = carry + lead;
    uint32_t tv, tn;
    if (pend >= 261u) {                                 // (at most once: pend <= 260 + 64)
      match_token(258u, kDrev, tv, tn);
      if (lane == cn) { cval = tv; cnb = tn; cpos = cbits; }
      cbits += tn; ++cn; pend -= 258u;
    }
    if (lead < 64u) {                                   // the run ends in this tile (or there is none)
      if (pend >= 259u) {
        match_token(pend - 3u, kDrev, tv, tn);
        if (lane == cn) { cval = tv; cnb = tn; cpos = cbits; }
        cbits += tn; ++cn;
        pend = 3u;
      }
      if (pend >= 3u) {
        match_token(pend, kDrev, tv, tn);
        if (lane == cn) { cval = tv; cnb = tn; cpos = cbits; }
        cbits += tn; ++cn;
      } else {
        // 1 or 2 bytes: literals; they lie in lanes lead - pend ... lead - 1 of this tile, or in
        // lanes 62, 63 of the last one (a remainder below 3 is a whole run: 258s leave >= 3)
        for (uint32_t k = pend; k >= 1u; --k) {
          const int at = (int)lead - (int)k;
          const uint32_t byte = at >= 0 ? (uint32_t)__shfl((int)v, at) : (uint32_t)__shfl((int)prevv, 64 + at);
          literal_token(byte, tv, tn);
          if (lane == cn) { cval = tv; cnb = tn; cpos = cbits; }
          cbits += tn; ++cn;
        }
      }
      pend = 0u;
    }

    // the lanes behind the carried run: literals, and the runs that start and end inside the tile
    uint32_t val = 0u, nb = 0u;
    uint32_t tail = 0u;                                 // lanes of the run open at the tile's end
    if (lead < 64u) {
      tail = (uint32_t)__builtin_clzll(~m);             // (~m != 0)
      if (valid && lane >= lead && lane < 64u - tail) {
        if (!eq) {
          literal_token(v, val, nb);
        } else {
          // lane `lead` is not in a run, so a stop lies below; the tail is excluded, so one lies above
          const uint64_t below = ~m & ((1ull << lane) - 1ull);
          const uint32_t start = 64u - (uint32_t)__builtin_clzll(below);
          const uint32_t stop = lane + (uint32_t)__builtin_ctzll(~m >> lane);
          const uint32_t L = stop - start;
          if (L < 3u) literal_token(v, val, nb);
          else if (lane == start) match_token(L, kDrev, val, nb);
        }
      }
    }
    carry = pend + tail;
    prevv = v;

    uint32_t inc = nb;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)inc, d);
      if (lane >= (uint32_t)d) inc += y;
    }
    const uint32_t lane_bits = (uint32_t)__shfl((int)inc, 63);
    put_bits(bits, r + cpos, cval, cnb);
    put_bits(bits, r + cbits + inc - nb, val, nb);
    __syncthreads();
    const uint32_t total = r + cbits + lane_bits;
    const uint32_t full = total >> 5;                   // <= 20
    const uint32_t word = bits[lane & 31u];
    const uint32_t rest = bits[full & 31u];
    __syncthreads();
    if (lane < full && wpos + lane < slot_words) out[wpos + lane] = word;
    if (lane < (uint32_t)kBitWords) bits[lane] = lane == 0u ? rest : 0u;
    __syncthreads();
    wpos += full;
    r = total & 31u;
  }

  // end of block (7 zero bits), empty stored block (3 zero bits, pad, 00 00 FF FF); behind the last
  // strip the final empty stored block (BFINAL = 1)
  r += 10u;
  r = (r + 7u) & ~7u;
  if (lane == 0u) put_bits(bits, r, 0xFFFF0000u, 32u);
  r += 32u;
  if (s == strips - 1) {
    if (lane == 0u) {
      put_bits(bits, r, 1u, 8u);
      put_bits(bits, r + 8u, 0xFFFF0000u, 32u);
    }
    r += 40u;
  }
  __syncthreads();
  const uint32_t bytes = r >> 3, words = (bytes + 3u) >> 2;       // <= 4 dwords
  if (lane < words && wpos + lane < slot_words) out[wpos + lane] = bits[lane];

#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    s1 += (uint32_t)__shfl_xor((int)s1, d);             // <= 64 lanes x 769 tiles x 255
    s2 += (uint32_t)__shfl_xor((int)s2, d);             // <= 64 x 65520
  }
  if (lane == 0u) {
    // (the clamp never acts: strip_bound() is what the tokens above can make at most; it keeps the
    // later passes inside `data` whatever this one did)
    const uint32_t most = (9u * n + 20u) / 8u + 4u + (s == strips - 1 ? 5u : 0u);
    const uint32_t made = wpos * 4u + bytes;
    rec[slot] = make_uint4(made < most ? made : most, s1 % kAdler, s2 % kAdler, 0u);
  }
}

// ---- layout ---------------------------------------------------------------------------------------
__device__ __forceinline__ void store_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
__device__ __forceinline__ uint32_t crc_step_bitwise(uint32_t crc, uint32_t byte) {
  crc ^= byte;
#pragma unroll
  for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
  return crc;
}

__device__ __forceinline__ uint64_t block_sum(uint64_t* red, uint64_t v) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const uint64_t total = red[0];
  __syncthreads();
  return total;
}

// grid (m), 256 threads; strips <= 1024 (kMaxSide / kRows)
__global__ __launch_bounds__(256) void png_layout_kernel(const uint4* __restrict__ rec, int H, int W,
                                                         int bpp, int depth, int color, int strips,
                                                         int64_t* __restrict__ dst,
                                                         uint32_t* __restrict__ adler,
                                                         uint8_t* __restrict__ data,
                                                         int64_t* __restrict__ offsets) {
  __shared__ uint64_t red[256];
  __shared__ uint32_t scan[256];
  const int tid = threadIdx.x, img = blockIdx.x, m = gridDim.x;
  const int64_t fixed = 51 + 12 * (int64_t)strips;

  uint64_t acc = 0;
  for (long j = tid; j < (long)img * strips; j += 256) acc += rec[j].x;
  const int64_t start = (int64_t)img * fixed + (int64_t)block_sum(red, acc);

  const int per = (strips + 255) / 256;
  const int lo = tid * per;
  uint32_t mine = 0u;
  uint64_t sums = 0;                                    // s1 in the low half, s2 in the high half
  for (int k = 0; k < per; ++k) {
    if (lo + k < strips) {
      const uint4 q = rec[(long)img * strips + lo + k];
      mine += q.x;
      sums += (uint64_t)q.y | ((uint64_t)q.z << 32);     // <= 1024 x 65520 each: no carry across
    }
  }
  scan[tid] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const uint32_t add = tid >= o ? scan[tid - o] : 0u;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const uint32_t own_total = scan[255];
  uint32_t run = scan[tid] - mine;
  for (int k = 0; k < per; ++k) {
    const int s = lo + k;
    if (s < strips) {
      dst[(long)img * strips + s] = start + 33 + 12 * (int64_t)s + (s > 0 ? 2 : 0) + run;
      run += rec[(long)img * strips + s].x;
    }
  }
  const uint64_t both = block_sum(red, sums);
  if (tid == 0) {
    const uint32_t rowlen = 1u + (uint32_t)W * bpp;
    const uint32_t N = (uint32_t)H * rowlen;
    const uint32_t A = (1u + (uint32_t)(both & 0xFFFFFFFFull)) % kAdler;
    const uint32_t B = (N % kAdler + (uint32_t)(both >> 32)) % kAdler;
    adler[img] = (B << 16) | A;
    offsets[img] = start;
    const int64_t end = start + fixed + own_total;
    if (img == m - 1) offsets[m] = end;
    uint8_t* f = data + start;
    store_be32(f, 0x89504E47u);
    store_be32(f + 4, 0x0D0A1A0Au);
    store_be32(f + 8, 13u);
    f[12] = 'I'; f[13] = 'H'; f[14] = 'D'; f[15] = 'R';
    store_be32(f + 16, (uint32_t)W);
    store_be32(f + 20, (uint32_t)H);
    f[24] = (uint8_t)depth; f[25] = (uint8_t)color; f[26] = 0; f[27] = 0; f[28] = 0;
    uint32_t crc = 0xFFFFFFFFu;
    for (int k = 12; k < 29; ++k) crc = crc_step_bitwise(crc, f[k]);
    store_be32(f + 29, ~crc);
    uint8_t* e = data + end - 12;
    store_be32(e, 0u);
    e[4] = 'I'; e[5] = 'E'; e[6] = 'N'; e[7] = 'D';
    store_be32(e + 8, 0xAE426082u);
  }
}

// ---- assemble -------------------------------------------------------------------------------------
// grid (ceil(strips / 4), m), 256 threads: wave = strip
__global__ __launch_bounds__(256) void png_assemble_kernel(const uint4* __restrict__ rec,
                                                           const int64_t* __restrict__ dst,
                                                           const uint32_t* __restrict__ adler,
                                                           const uint8_t* __restrict__ slots,
                                                           uint32_t slot_bytes, int strips,
                                                           uint8_t* __restrict__ data) {
  __shared__ uint32_t table[256];
  {
    uint32_t c = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    table[threadIdx.x] = c;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), img = blockIdx.y;
  if (s >= strips) return;
  const size_t slot = (size_t)img * strips + s;
  uint32_t bytes = rec[slot].x;
  if (bytes > slot_bytes) bytes = slot_bytes;           // (never: the slot is sized for the worst case)
  const uint8_t* from = slots + slot * slot_bytes;
  const bool first = s == 0, last = s == strips - 1;
  uint8_t* chunk = data + dst[slot];
  uint8_t* body = chunk + 8 + (first ? 2 : 0);
  for (uint32_t j = lane; j < bytes; j += 64u) body[j] = from[j];
  if (lane == 0) {
    store_be32(chunk, bytes + (first ? 2u : 0u) + (last ? 4u : 0u));
    chunk[4] = 'I'; chunk[5] = 'D'; chunk[6] = 'A'; chunk[7] = 'T';
    uint32_t crc = 0xFFFFFFFFu;
    crc = table[(crc ^ 'I') & 0xFFu] ^ (crc >> 8);
    crc = table[(crc ^ 'D') & 0xFFu] ^ (crc >> 8);
    crc = table[(crc ^ 'A') & 0xFFu] ^ (crc >> 8);
    crc = table[(crc ^ 'T') & 0xFFu] ^ (crc >> 8);
    if (first) {
      chunk[8] = 0x78; chunk[9] = 0x01;
      crc = table[(crc ^ 0x78u) & 0xFFu] ^ (crc >> 8);
      crc = table[(crc ^ 0x01u) & 0xFFu] ^ (crc >> 8);
    }
    const uint32_t* fw = reinterpret_cast<const uint32_t*>(from);
    const uint32_t whole = bytes >> 2;
    for (uint32_t j = 0; j < whole; ++j) {
      const uint32_t wd = fw[j];
      crc = table[(crc ^ wd) & 0xFFu] ^ (crc >> 8);
      crc = table[(crc ^ (wd >> 8)) & 0xFFu] ^ (crc >> 8);
      crc = table[(crc ^ (wd >> 16)) & 0xFFu] ^ (crc >> 8);
      crc = table[(crc ^ (wd >> 24)) & 0xFFu] ^ (crc >> 8);
    }
    for (uint32_t j = whole << 2; j < bytes; ++j) crc = table[(crc ^ from[j]) & 0xFFu] ^ (crc >> 8);
    uint8_t* end = body + bytes;
    if (last) {
      const uint32_t ad = adler[img];
      store_be32(end, ad);
      for (int k = 24; k >= 0; k -= 8) crc = table[(crc ^ (ad >> k)) & 0xFFu] ^ (crc >> 8);
      end += 4;
    }
    store_be32(end, ~crc);
  }
}

inline bool geometry_ok(int layout, int m, int h, int w) {
  return layout >= EMSA_PNG_GRAY8 && layout <= EMSA_PNG_GRAY16 && m >= 1 && m <= 65535 && h >= 1 &&
         h <= kMaxSide && w >= 1 && w <= kMaxSide;
}

}  // namespace

extern "C" int64_t emsa_png_bound(int32_t layout, int32_t h, int32_t w) {
  if (!geometry_ok(layout, 1, h, w)) return EMSA_E_SHAPE;
  return geometry(layout, h, w).bound;
}

extern "C" int64_t emsa_png_ws_bytes(int32_t layout, int32_t m, int32_t h, int32_t w) {
  if (!geometry_ok(layout, m, h, w)) return EMSA_E_SHAPE;
  return workspace(geometry(layout, h, w), m).total;
}

extern "C" int emsa_png_encode(const void* src, int32_t layout, int32_t m, int32_t h, int32_t w,
                               uint8_t* data, int64_t data_bytes, int64_t* offsets, void* ws,
                               void* stream) {
  if (!geometry_ok(layout, m, h, w)) return EMSA_E_SHAPE;
  const Geo g = geometry(layout, h, w);
  if (data_bytes < (int64_t)m * g.bound) return EMSA_E_SHAPE;
  if (!src || !data || !offsets || !ws) return EMSA_E_ARG;
  if ((uintptr_t)ws % 16 || (uintptr_t)offsets % 8) return EMSA_E_ARG;
  const Ws l = workspace(g, m);
  uint8_t* base = (uint8_t*)ws;
  uint4* rec = (uint4*)(base + l.rec);
  int64_t* dst = (int64_t*)(base + l.dst);
  uint32_t* adler = (uint32_t*)(base + l.adler);
  uint8_t* slots = base + l.slots;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.strips, m);
  const uint8_t* in = (const uint8_t*)src;
  if (layout == EMSA_PNG_GRAY8)
    hipLaunchKernelGGL(png_strip_kernel<1>, grid, dim3(64), 0, st, in, h, w, g.strips,
                       (uint32_t)g.slot_bytes, rec, slots);
  else if (layout == EMSA_PNG_BGR8)
    hipLaunchKernelGGL(png_strip_kernel<3>, grid, dim3(64), 0, st, in, h, w, g.strips,
                       (uint32_t)g.slot_bytes, rec, slots);
  else
    hipLaunchKernelGGL(png_strip_kernel<2>, grid, dim3(64), 0, st, in, h, w, g.strips,
                       (uint32_t)g.slot_bytes, rec, slots);
  hipLaunchKernelGGL(png_layout_kernel, dim3(m), dim3(256), 0, st, rec, h, w, g.bpp,
                     layout == EMSA_PNG_GRAY16 ? 16 : 8, layout == EMSA_PNG_BGR8 ? 2 : 0, g.strips, dst,
                     adler, data, offsets);
  hipLaunchKernelGGL(png_assemble_kernel, dim3((g.strips + 3) / 4, m), dim3(256), 0, st, rec, dst,
                     adler, slots, (uint32_t)g.slot_bytes, g.strips, data);
  return emsa_launch_status();
}
