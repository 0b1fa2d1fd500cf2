// The decode core of csrc/png_decode.hip: chunk walk, bit reader, Huffman table builder with its
// validation, the inflate loop with its bounds logic, Adler-32 and the filter arithmetic.
// ONE text, two builds:
//   * with PNGD_DEVICE defined (png_decode.hip) it is device code for one wave of 64 lanes: control
//     flow and every decoded value are the same in all lanes, the lanes share the byte copies, the
//     table fills and the checksum;
//   * without it (tools/png_decode_host.cpp) it is plain C++ with one "lane", compiled under
//     AddressSanitizer / UBSan and fed the malformed corpus of tests/test_png_decode.py -- bounds
//     mistakes are found there, on the CPU, before a stream reaches a GPU.
// Termination on arbitrary bytes: every loop iteration below either consumes input (bits of a stream
// of zlen bytes, checked with pngd_over() -- the reader hands out zero bits past the end, at most
// 64 + 48 of them before the check trips -- or >= 12 bytes of a file of flen bytes) or produces
// output bytes against the hard size `cap`; an iteration that can do neither returns a status.
// Memory: reads only f[0, flen) / z[0, zlen) / out[0, cap) once complete; writes only z[0, zcap) and
// out[0, cap).
// Chunk CRC-32s are not verified.
#ifndef EMSA_PNG_INFLATE_CORE_H
#define EMSA_PNG_INFLATE_CORE_H
#include <stdint.h>

#include "emsanet_hip.h"

#ifdef PNGD_DEVICE
#define PNGD_FN __device__ __forceinline__
#define PNGD_HD __host__ __device__ __forceinline__
#define PNGD_NL 64u
#define PNGD_LANE ((uint32_t)threadIdx.x)
#define PNGD_SYNC() __syncthreads()
#define PNGD_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define PNGD_WAVE_ORDER() __builtin_amdgcn_wave_barrier()
#else
#define PNGD_FN static inline
#define PNGD_HD static inline
#define PNGD_NL 1u
#define PNGD_LANE 0u
#define PNGD_SYNC() ((void)0)
#define PNGD_UNI(x) ((uint32_t)(x))
#define PNGD_WAVE_ORDER() ((void)0)
#endif

#define PNGD_NOSYM 0xFFFFu
#define PNGD_WINDOW 32768u
#define PNGD_ADLER_MOD 65521u

// ---- wave operations (identity with one lane) -------------------------------------------------------
PNGD_FN uint64_t pngd_ballot(bool p) {
#ifdef PNGD_DEVICE
  return __ballot(p);
#else
  return p ? 1ull : 0ull;
#endif
}
PNGD_FN uint32_t pngd_popc(uint64_t v) {
#ifdef PNGD_DEVICE
  return (uint32_t)__popcll(v);
#else
  return (uint32_t)__builtin_popcountll(v);
#endif
}
PNGD_FN uint32_t pngd_wave_sum(uint32_t v) {
#ifdef PNGD_DEVICE
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
#endif
  return v;
}
PNGD_FN uint32_t pngd_rev(uint32_t code, uint32_t len) {       // len in 1 ... 15
#ifdef PNGD_DEVICE
  return __brev(code) >> (32u - len);
#else
  uint32_t r = 0u;
  for (uint32_t k = 0u; k < len; ++k) { r = (r << 1) | (code & 1u); code >>= 1; }
  return r;
#endif
}
PNGD_FN uint32_t pngd_be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// ---- geometry ---------------------------------------------------------------------------------------
PNGD_HD int pngd_bpp(int layout) { return layout == EMSA_PNG_BGR8 ? 3 : (layout == EMSA_PNG_GRAY16 ? 2 : 1); }
// how a byte of an unfiltered row (file order) lands in the output row: 0 as it is, 1 the three bytes
// of a pixel reversed (R,G,B -> B,G,R), 2 the two bytes of a sample swapped (big-endian -> host)
PNGD_HD int pngd_store_mode(int layout, int order) {
  return layout == EMSA_PNG_GRAY16 ? 2 : (layout == EMSA_PNG_BGR8 && order == EMSA_PNGD_BGR ? 1 : 0);
}
PNGD_HD uint32_t pngd_out_col(int mode, uint32_t col) {
  if (mode == 2) return col ^ 1u;
  if (mode == 1) { const uint32_t px = col / 3u; return 6u * px + 2u - col; }
  return col;
}

// ---- filters ----------------------------------------------------------------------------------------
// the predictor of filter type f (0 ... 4) from the bytes left (a), above (b) and above left (c)
PNGD_HD uint32_t pngd_predict(uint32_t f, uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  int pa = p - (int)a, pb = p - (int)b, pc = p - (int)c;
  pa = pa < 0 ? -pa : pa; pb = pb < 0 ? -pb : pb; pc = pc < 0 ? -pc : pc;
  const uint32_t paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  return f == 1u ? a : f == 2u ? b : f == 3u ? ((a + b) >> 1) : f == 4u ? paeth : 0u;
}

// ---- chunk walk -------------------------------------------------------------------------------------
// signature, IHDR (against the call), then every chunk up to IEND: IDAT payloads are joined into
// z[0, *zlen) by all lanes, everything else is skipped where it stands.  IDAT chunks must be
// consecutive and IEND must end the file.
PNGD_FN int pngd_walk(const uint8_t* f, uint32_t flen, int layout, int h, int w, uint8_t* z,
                      uint32_t zcap, uint32_t* zlen) {
  const uint32_t lane = PNGD_LANE;
  *zlen = 0u;
  if (flen < 8u + 25u + 12u) return EMSA_PNGD_CHUNK;
  if (pngd_be32(f) != 0x89504E47u || pngd_be32(f + 4) != 0x0D0A1A0Au) return EMSA_PNGD_CHUNK;
  if (pngd_be32(f + 8) != 13u || pngd_be32(f + 12) != 0x49484452u) return EMSA_PNGD_CHUNK;
  const uint32_t depth = layout == EMSA_PNG_GRAY16 ? 16u : 8u, color = layout == EMSA_PNG_BGR8 ? 2u : 0u;
  if (pngd_be32(f + 16) != (uint32_t)w || pngd_be32(f + 20) != (uint32_t)h || f[24] != depth ||
      f[25] != color || f[26] != 0u || f[27] != 0u || f[28] != 0u)
    return EMSA_PNGD_IHDR;
  uint32_t pos = 33u, n = 0u;
  int idat = 0;                                      // 0 none yet, 1 inside the run, 2 behind it
  for (;;) {                                         // each turn takes >= 12 bytes of flen
    if (flen - pos < 12u) return EMSA_PNGD_CHUNK;
    const uint32_t len = pngd_be32(f + pos), type = pngd_be32(f + pos + 4u);
    if (len > flen - pos - 12u) return EMSA_PNGD_CHUNK;
    if (type == 0x49454E44u) {                       // IEND
      if (len != 0u || pos + 12u != flen || idat == 0) return EMSA_PNGD_CHUNK;
      break;
    }
    if (type == 0x49484452u) return EMSA_PNGD_CHUNK; // a second IHDR
    if (type == 0x49444154u) {                       // IDAT
      if (idat == 2 || len > zcap - n) return EMSA_PNGD_CHUNK;
      idat = 1;
      const uint8_t* src = f + pos + 8u;
      for (uint32_t i = lane; i < len; i += PNGD_NL) z[n + i] = src[i];
      n += len;
    } else if (idat == 1) {
      idat = 2;
    }
    pos += 12u + len;
  }
  *zlen = n;
  return EMSA_PNGD_OK;
}

// ---- bit reader -------------------------------------------------------------------------------------
// LSB-first over z[0, zlen), zero bits behind the end; `k` counts the dwords taken, so the bits
// consumed are 32 k - cnt.  Device: each lane holds one dword of the current and of the next block of
// 64 dwords (`z` is 4-byte aligned there), a refill is a lane read -- no memory latency inside the
// symbol loop.
struct PngdBits {
  const uint8_t* z;
  uint32_t zlen, cnt, k;
  uint64_t buf;
#ifdef PNGD_DEVICE
  uint32_t cur, nxt;
#endif
};
PNGD_FN uint32_t pngd_load_word(const uint8_t* z, uint32_t zlen, uint32_t idx) {
  if (idx >= 0x40000000u) return 0u;
  const uint32_t o = idx * 4u;
  if (o >= zlen) return 0u;
#ifdef PNGD_DEVICE
  if (zlen - o >= 4u) return *reinterpret_cast<const uint32_t*>(z + o);
#endif
  uint32_t r = 0u;
  for (uint32_t j = 0u; j < 4u && o + j < zlen; ++j) r |= (uint32_t)z[o + j] << (8u * j);
  return r;
}
PNGD_FN uint32_t pngd_word(PngdBits& b) {
#ifdef PNGD_DEVICE
  const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)b.cur, (int)PNGD_UNI(b.k & 63u));
  ++b.k;
  if ((b.k & 63u) == 0u) {
    b.cur = b.nxt;
    b.nxt = pngd_load_word(b.z, b.zlen, b.k + 64u + PNGD_LANE);
  }
  return w;
#else
  return pngd_load_word(b.z, b.zlen, b.k++);
#endif
}
PNGD_FN void pngd_seek(PngdBits& b, uint32_t bytepos) {
  b.k = bytepos >> 2;
#ifdef PNGD_DEVICE
  const uint32_t base = b.k & ~63u;
  b.cur = pngd_load_word(b.z, b.zlen, base + PNGD_LANE);
  b.nxt = pngd_load_word(b.z, b.zlen, base + 64u + PNGD_LANE);
#endif
  const uint32_t sh = 8u * (bytepos & 3u);
  b.buf = (uint64_t)(pngd_word(b) >> sh);
  b.cnt = 32u - sh;
}
PNGD_FN void pngd_need(PngdBits& b) {                 // -> at least 33 bits in buf
  if (b.cnt <= 32u) {
    b.buf |= (uint64_t)pngd_word(b) << b.cnt;
    b.cnt += 32u;
  }
}
PNGD_FN void pngd_drop(PngdBits& b, uint32_t n) { b.buf >>= n; b.cnt -= n; }
PNGD_FN uint32_t pngd_take(PngdBits& b, uint32_t n) {  // n <= 16, n <= cnt
  const uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
  pngd_drop(b, n);
  return v;
}
PNGD_FN uint64_t pngd_used_bits(const PngdBits& b) { return (uint64_t)b.k * 32u - b.cnt; }
PNGD_FN bool pngd_over(const PngdBits& b) { return pngd_used_bits(b) > (uint64_t)b.zlen * 8u; }

// ---- Huffman tables (LDS on the device) -------------------------------------------------------------
// canonical code of up to 288 symbols: per length the number of codes, the first code and where its
// symbols start in `symbol` (sorted by length, then by value); `fast` resolves codes of up to `fb`
// bits in one lookup (entry = length << 9 | symbol, 0 = longer or unused).
struct PngdHuff {
  uint16_t count[16], first[16], offs[16], run[16];
  uint16_t symbol[288];
  uint16_t fast[1024];
};
struct PngdTables {
  PngdHuff lit, dist, cl;
  uint8_t len[320];           // literal/length then distance code lengths of the block
  uint8_t cllen[32];          // the 19 lengths of the code-length code
  uint8_t win[PNGD_WINDOW];   // the last 32 KiB of output: byte p at win[p % 32768]
};

// lens[0, n) -> h.  false: over-subscribed, or incomplete (allowed only with `single`: no code at all,
// or one code of length 1 -- the distance tree of a block with one distance).  All lanes fill.
PNGD_FN bool pngd_build(PngdHuff& h, const uint8_t* lens, uint32_t n, uint32_t fb, bool single) {
  const uint32_t lane = PNGD_LANE;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t i = lane; i < 16u; i += PNGD_NL) h.count[i] = 0;
  for (uint32_t i = lane; i < (1u << fb); i += PNGD_NL) h.fast[i] = 0;
  PNGD_SYNC();
  for (uint32_t base = 0u; base < n; base += PNGD_NL) {
    const uint32_t s = base + lane, l = s < n ? lens[s] : 0u;
    for (uint32_t L = 1u; L <= 15u; ++L) {
      const uint64_t m = pngd_ballot(l == L);
      if (lane == 0u && m) h.count[L] = (uint16_t)(h.count[L] + pngd_popc(m));
    }
  }
  PNGD_SYNC();
  int left = 1;
  uint32_t code = 0u, total = 0u, longest = 0u;
  for (uint32_t L = 1u; L <= 15u; ++L) {
    const uint32_t c = PNGD_UNI(h.count[L]);
    left = (left << 1) - (int)c;
    if (left < 0) return false;
    if (lane == 0u) { h.first[L] = (uint16_t)code; h.offs[L] = (uint16_t)total; h.run[L] = (uint16_t)total; }
    code = (code + c) << 1;
    total += c;
    if (c) longest = L;
  }
  if (left > 0 && !(single && total <= 1u && longest <= 1u)) return false;
  PNGD_SYNC();
  for (uint32_t base = 0u; base < n; base += PNGD_NL) {
    const uint32_t s = base + lane, l = s < n ? lens[s] : 0u;
    uint32_t rank = 0u, tot = 0u;
    for (uint32_t L = 1u; L <= 15u; ++L) {
      const uint64_t m = pngd_ballot(l == L);
      if (l == L) { rank = pngd_popc(m & below); tot = pngd_popc(m); }
    }
    const uint32_t at = l ? h.run[l] : 0u;
    PNGD_SYNC();
    if (l) {
      h.symbol[at + rank] = (uint16_t)s;             // at + rank < total <= n <= 288
      if (rank + 1u == tot) h.run[l] = (uint16_t)(at + tot);
    }
    PNGD_SYNC();
  }
  for (uint32_t i = lane; i < total; i += PNGD_NL) {
    const uint32_t s = h.symbol[i], l = lens[s];
    if (l <= fb) {
      const uint32_t r = pngd_rev(h.first[l] + (i - h.offs[l]), l);
      for (uint32_t j = r; j < (1u << fb); j += 1u << l) h.fast[j] = (uint16_t)((l << 9) | s);
    }
  }
  PNGD_SYNC();
  return true;
}

// one symbol off the reader (>= 15 bits in buf), PNGD_NOSYM when no code matches
PNGD_FN uint32_t pngd_decode(const PngdHuff& h, uint32_t fb, PngdBits& b) {
  const uint32_t e = PNGD_UNI(h.fast[(uint32_t)b.buf & ((1u << fb) - 1u)]);
  if (e) {
    pngd_drop(b, e >> 9);
    return e & 511u;
  }
  uint32_t code = 0u, bits = (uint32_t)b.buf;
  for (uint32_t L = 1u; L <= 15u; ++L) {
    code |= bits & 1u;
    bits >>= 1;
    const uint32_t c = PNGD_UNI(h.count[L]), f = PNGD_UNI(h.first[L]);
    if (code >= f && code - f < c) {
      pngd_drop(b, L);
      return PNGD_UNI(h.symbol[PNGD_UNI(h.offs[L]) + code - f]);
    }
    code <<= 1;
  }
  return PNGD_NOSYM;
}

// ---- inflate ----------------------------------------------------------------------------------------
// the literals gathered one per lane -> out and the window (pos + npend <= cap is the caller's)
PNGD_FN void pngd_flush(uint8_t* out, uint8_t* win, uint32_t& pos, uint32_t& npend, uint32_t pend) {
  if (PNGD_LANE < npend) {
    out[pos + PNGD_LANE] = (uint8_t)pend;
    win[(pos + PNGD_LANE) & (PNGD_WINDOW - 1u)] = (uint8_t)pend;
  }
  pos += npend;
  npend = 0u;
}

// zlib stream z[0, zlen) -> exactly cap bytes in out, Adler-32 checked.  Literals are gathered one per
// lane and stored together; a match is copied by all lanes, byte i from pos - dist + i % dist.  `out` is
// only written here (and read once, for the Adler-32): the window the matches read is T.win.
PNGD_FN int pngd_inflate(const uint8_t* z, uint32_t zlen, uint8_t* out, uint32_t cap, PngdTables& T) {
  const uint32_t lane = PNGD_LANE;
  if (zlen < 2u) return EMSA_PNGD_TRUNCATED;
  const uint32_t cmf = z[0], flg = z[1];
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u))
    return EMSA_PNGD_ZLIB_HEADER;
  PngdBits b;
  b.z = z;
  b.zlen = zlen;
  pngd_seek(b, 2u);
  uint32_t pos = 0u, npend = 0u, pend = 0u;
  bool last = false, fixed_ready = false;
  while (!last) {
    pngd_need(b);
    last = pngd_take(b, 1u) != 0u;
    const uint32_t type = pngd_take(b, 2u);
    if (pngd_over(b)) return EMSA_PNGD_TRUNCATED;
    if (type == 3u) return EMSA_PNGD_BLOCK_TYPE;
    if (type == 0u) {
      pngd_drop(b, b.cnt & 7u);
      const uint64_t at64 = pngd_used_bits(b) >> 3;
      if (at64 + 4u > zlen) return EMSA_PNGD_TRUNCATED;
      const uint32_t at = (uint32_t)at64;
      const uint32_t len = (uint32_t)z[at] | ((uint32_t)z[at + 1u] << 8);
      const uint32_t nlen = (uint32_t)z[at + 2u] | ((uint32_t)z[at + 3u] << 8);
      if ((len ^ 0xFFFFu) != nlen) return EMSA_PNGD_STORED_LEN;
      if (len > zlen - at - 4u) return EMSA_PNGD_TRUNCATED;
      if (len > cap - pos) return EMSA_PNGD_TOO_MANY;
      for (uint32_t i = lane; i < len; i += PNGD_NL) {
        const uint8_t v = z[at + 4u + i];
        out[pos + i] = v;
        T.win[(pos + i) & (PNGD_WINDOW - 1u)] = v;
      }
      pos += len;
      pngd_seek(b, at + 4u + len);
      continue;
    }
    if (type == 1u) {
      if (!fixed_ready) {
        PNGD_SYNC();
        for (uint32_t i = lane; i < 320u; i += PNGD_NL)
          T.len[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < 288u ? 8u : 5u);
        PNGD_SYNC();
        pngd_build(T.lit, T.len, 288u, 10u, false);
        pngd_build(T.dist, T.len + 288u, 32u, 8u, false);
        fixed_ready = true;
      }
    } else {
      fixed_ready = false;
      pngd_need(b);
      const uint32_t hlit = pngd_take(b, 5u) + 257u, hdist = pngd_take(b, 5u) + 1u;
      const uint32_t hclen = pngd_take(b, 4u) + 4u;
      if (pngd_over(b)) return EMSA_PNGD_TRUNCATED;
      if (hlit > 286u || hdist > 30u) return EMSA_PNGD_CODE_LENGTHS;
      PNGD_SYNC();
      for (uint32_t i = lane; i < 32u; i += PNGD_NL) T.cllen[i] = 0;
      PNGD_SYNC();
      for (uint32_t i = 0u; i < hclen; ++i) {
        pngd_need(b);
        const uint32_t v = pngd_take(b, 3u);
        // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
        const uint32_t where = i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? 8u - ((i - 3u) >> 1) : 7u + ((i - 2u) >> 1);
        if (lane == 0u) T.cllen[where] = (uint8_t)v;
      }
      if (pngd_over(b)) return EMSA_PNGD_TRUNCATED;
      PNGD_SYNC();
      if (!pngd_build(T.cl, T.cllen, 19u, 7u, false)) return EMSA_PNGD_CODE_LENGTHS;
      const uint32_t n = hlit + hdist;
      uint32_t i = 0u, prev = 0u;
      while (i < n) {                                // each turn takes >= 1 bit and advances i
        pngd_need(b);
        const uint32_t s = pngd_decode(T.cl, 7u, b);
        if (pngd_over(b)) return EMSA_PNGD_TRUNCATED;
        if (s > 18u) return EMSA_PNGD_CODE_LENGTHS;
        if (s < 16u) {
          if (lane == 0u) T.len[i] = (uint8_t)s;
          ++i;
          prev = s;
          continue;
        }
        if (s == 16u && i == 0u) return EMSA_PNGD_CODE_LENGTHS;
        const uint32_t val = s == 16u ? prev : 0u;
        const uint32_t rep = s == 16u ? 3u + pngd_take(b, 2u) : s == 17u ? 3u + pngd_take(b, 3u) : 11u + pngd_take(b, 7u);
        if (pngd_over(b)) return EMSA_PNGD_TRUNCATED;
        if (rep > n - i) return EMSA_PNGD_CODE_LENGTHS;
        for (uint32_t j = lane; j < rep; j += PNGD_NL) T.len[i + j] = (uint8_t)val;
        i += rep;
        prev = val;
      }
      PNGD_SYNC();
      if (PNGD_UNI(T.len[256]) == 0u) return EMSA_PNGD_CODE_LENGTHS;     // no end-of-block code
      if (!pngd_build(T.lit, T.len, hlit, 10u, false)) return EMSA_PNGD_CODE_LENGTHS;
      if (!pngd_build(T.dist, T.len + hlit, hdist, 8u, true)) return EMSA_PNGD_CODE_LENGTHS;
    }
    const uint64_t end_bits = (uint64_t)zlen * 8u;
    for (;;) {                                       // each turn takes >= 1 bit
      // a run of literals with short codes, the common case, as a loop of its own: one table lookup,
      // no other branch.  Whatever it cannot take (a long code, a length, no room, the end of the
      // input) is left unconsumed for the general path below, which names the error.
      for (;;) {
        pngd_need(b);
        const uint32_t e = PNGD_UNI(T.lit.fast[(uint32_t)b.buf & 1023u]);
        if (e == 0u || (e & 256u) || npend >= cap - pos) break;
        if (pngd_used_bits(b) + (e >> 9) > end_bits) break;
        pngd_drop(b, e >> 9);
        if (lane == npend) pend = e & 255u;
        if (++npend == PNGD_NL) pngd_flush(out, T.win, pos, npend, pend);
      }
      pngd_need(b);
      const uint32_t sym = pngd_decode(T.lit, 10u, b);
      if (pngd_over(b)) return EMSA_PNGD_TRUNCATED;
      if (sym == PNGD_NOSYM || sym > 285u) return EMSA_PNGD_SYMBOL;
      if (sym < 256u) {
        if (npend >= cap - pos) return EMSA_PNGD_TOO_MANY;
        if (lane == npend) pend = sym;
        if (++npend < PNGD_NL) continue;
      }
      pngd_flush(out, T.win, pos, npend, pend);
      if (sym < 256u) continue;
      if (sym == 256u) break;
      uint32_t len;
      if (sym < 265u) len = sym - 254u;
      else if (sym == 285u) len = 258u;
      else {
        const uint32_t e = (sym - 261u) >> 2;
        len = 3u + ((4u + ((sym - 261u) & 3u)) << e) + pngd_take(b, e);
      }
      pngd_need(b);
      const uint32_t ds = pngd_decode(T.dist, 8u, b);
      if (ds == PNGD_NOSYM || ds > 29u) return pngd_over(b) ? EMSA_PNGD_TRUNCATED : EMSA_PNGD_SYMBOL;
      uint32_t dist = ds + 1u;
      if (ds >= 4u) {
        const uint32_t e = (ds - 2u) >> 1;
        dist = 1u + ((2u + (ds & 1u)) << e) + pngd_take(b, e);
      }
      if (pngd_over(b)) return EMSA_PNGD_TRUNCATED;
      if (dist > pos) return EMSA_PNGD_DISTANCE;
      if (len > cap - pos) return EMSA_PNGD_TOO_MANY;
      // The source is the window, not `out`: a wave's LDS accesses execute in program order, so the
      // bytes the lanes have just stored are there without waiting for global memory.  Byte i of the
      // match lands on the slot of source byte i + (32768 - dist) at the earliest: never on one that
      // is still to be read (dist >= len there, so the lanes read source byte i itself).
      PNGD_WAVE_ORDER();
      for (uint32_t i = lane; i < len; i += PNGD_NL) {
        const uint8_t v = T.win[(pos - dist + (dist < len ? i % dist : i)) & (PNGD_WINDOW - 1u)];
        out[pos + i] = v;
        T.win[(pos + i) & (PNGD_WINDOW - 1u)] = v;
      }
      pos += len;
    }
  }
  if (pos != cap) return EMSA_PNGD_TOO_FEW;
  const uint64_t end = (pngd_used_bits(b) + 7u) >> 3;
  if (end + 4u > zlen) return EMSA_PNGD_TRUNCATED;
  const uint32_t stored = pngd_be32(z + (uint32_t)end);
  PNGD_SYNC();
  // A = 1 + sum f[i], B = cap + sum (cap - i) f[i]: a partial sum per lane, as the encoder forms them;
  // 64-bit sums need no reduction on the way (255 * cap * cap / lanes < 2^64 for cap <= 4096 * 12289)
  uint64_t s1 = 0u, s2 = 0u;
  for (uint32_t i = lane; i < cap; i += PNGD_NL) {
    const uint32_t v = out[i];
    s1 += v;
    s2 += (uint64_t)v * (cap - i);
  }
  const uint32_t A = (1u + pngd_wave_sum((uint32_t)(s1 % PNGD_ADLER_MOD))) % PNGD_ADLER_MOD;
  const uint32_t B = (cap % PNGD_ADLER_MOD + pngd_wave_sum((uint32_t)(s2 % PNGD_ADLER_MOD))) % PNGD_ADLER_MOD;
  return ((B << 16) | A) == stored ? EMSA_PNGD_OK : EMSA_PNGD_ADLER;
}

#ifndef PNGD_DEVICE
// ---- the host build's unfilter: the plain double loop ------------------------------------------------
// scan: h rows of 1 + stride bytes -> dst h rows of stride bytes in the output layout
static inline int pngd_unfilter_host(uint8_t* scan, int h, uint32_t stride, int bpp, int mode, uint8_t* dst) {
  const uint32_t rowlen = 1u + stride;
  for (int y = 0; y < h; ++y)
    if (scan[(uint64_t)y * rowlen] > 4u) return EMSA_PNGD_FILTER;
  for (int y = 0; y < h; ++y) {
    uint8_t* cur = scan + (uint64_t)y * rowlen + 1u;
    const uint8_t* up = y ? cur - rowlen : nullptr;
    const uint32_t f = cur[-1];
    for (uint32_t x = 0u; x < stride; ++x) {
      const uint32_t a = x >= (uint32_t)bpp ? cur[x - bpp] : 0u;
      const uint32_t bb = up ? up[x] : 0u;
      const uint32_t c = (up && x >= (uint32_t)bpp) ? up[x - bpp] : 0u;
      cur[x] = (uint8_t)(cur[x] + pngd_predict(f, a, bb, c));
      dst[(uint64_t)y * stride + pngd_out_col(mode, x)] = cur[x];
    }
  }
  return EMSA_PNGD_OK;
}
#endif

#endif  // EMSA_PNG_INFLATE_CORE_H
