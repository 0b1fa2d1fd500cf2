// The host build of csrc/png_inflate_core.h: the decode core of csrc/png_decode.hip as plain C++ with
// one lane, in a stand-alone program.  tests/test_png_decode.py compiles it with
// -fsanitize=address,undefined and runs it over its whole corpus, valid and malformed: every buffer
// here is a heap block of exactly the size the device code is given (file, joined stream, scanlines,
// image), so a read or write one byte outside is reported.
//
//   png_decode_host CORPUS [IMAGES]
// CORPUS: "PNGDCORP", int32 count, then per entry int32 layout, order, h, w, int64 bytes, the file.
// Output: one line "index status crc32-of-image" per entry; IMAGES receives the decoded images back to
// back (all zero for a failed file), in the layout emsa_png_decode writes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../emsanet_amd/csrc/png_inflate_core.h"

static uint32_t crc32_of(const uint8_t* p, size_t n) {
  uint32_t crc = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
  }
  return ~crc;
}

static int decode_one(const uint8_t* file, uint32_t flen, int layout, int order, int h, int w, uint8_t* image) {
  const int bpp = pngd_bpp(layout);
  const uint32_t stride = (uint32_t)w * (uint32_t)bpp, cap = (uint32_t)h * (1u + stride);
  uint8_t* z = (uint8_t*)malloc(flen ? flen : 1u);
  uint8_t* scan = (uint8_t*)malloc(cap);
  PngdTables* tables = (PngdTables*)malloc(sizeof(PngdTables));
  uint32_t zlen = 0u;
  int st = pngd_walk(file, flen, layout, h, w, z, flen, &zlen);
  if (st == EMSA_PNGD_OK) {
    // the stream in a block of its own size: a read behind zlen is a finding
    uint8_t* zz = (uint8_t*)malloc(zlen ? zlen : 1u);
    memcpy(zz, z, zlen);
    st = pngd_inflate(zz, zlen, scan, cap, *tables);
    free(zz);
  }
  if (st == EMSA_PNGD_OK) st = pngd_unfilter_host(scan, h, stride, bpp, pngd_store_mode(layout, order), image);
  if (st != EMSA_PNGD_OK) memset(image, 0, (size_t)h * stride);
  free(tables);
  free(scan);
  free(z);
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s CORPUS [IMAGES]\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { perror(argv[1]); return 2; }
  FILE* out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
  if (argc > 2 && !out) { perror(argv[2]); return 2; }
  char magic[8];
  int32_t count = 0;
  if (fread(magic, 1, 8, in) != 8 || memcmp(magic, "PNGDCORP", 8) || fread(&count, 4, 1, in) != 1 || count < 0) {
    fprintf(stderr, "%s: not a corpus file\n", argv[1]);
    return 2;
  }
  for (int32_t i = 0; i < count; ++i) {
    int32_t head[4];
    int64_t bytes = 0;
    if (fread(head, 4, 4, in) != 4 || fread(&bytes, 8, 1, in) != 1 || bytes < 0 || bytes > ((int64_t)1 << 30)) {
      fprintf(stderr, "entry %d: bad header\n", i);
      return 2;
    }
    const int layout = head[0], order = head[1], h = head[2], w = head[3];
    if (layout < EMSA_PNG_GRAY8 || layout > EMSA_PNG_GRAY16 || (order != EMSA_PNGD_RGB && order != EMSA_PNGD_BGR) ||
        h < 1 || h > EMSA_PNG_MAX_SIDE || w < 1 || w > EMSA_PNG_MAX_SIDE) {
      fprintf(stderr, "entry %d: bad geometry\n", i);
      return 2;
    }
    uint8_t* file = (uint8_t*)malloc(bytes ? (size_t)bytes : 1u);
    if (fread(file, 1, (size_t)bytes, in) != (size_t)bytes) {
      fprintf(stderr, "entry %d: short read\n", i);
      return 2;
    }
    const size_t image_bytes = (size_t)h * w * pngd_bpp(layout);
    uint8_t* image = (uint8_t*)malloc(image_bytes);
    const int st = decode_one(file, (uint32_t)bytes, layout, order, h, w, image);
    printf("%d %d %08x\n", i, st, crc32_of(image, image_bytes));
    if (out && fwrite(image, 1, image_bytes, out) != image_bytes) { perror("write"); return 2; }
    free(image);
    free(file);
  }
  if (out) fclose(out);
  fclose(in);
  return 0;
}
