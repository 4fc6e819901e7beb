// jpeg_encode_host.h -- the serial half of the baseline JPEG encoder: the Huffman (entropy) stage over quantised coefficients
// in the decoder's layout (csrc/jpeg_host.h), in plain C++ with no HIP call, so that a stand-alone program can run it under a
// sanitiser (tools/jpeg_encode_host_check.cpp).  Included by csrc/jpeg_encode.hip, whose device path it defines byte for byte.
//
// Every output byte goes through Sink::put, which counts always and stores only below the capacity, so the needed length of a
// stream that does not fit is still known; the coefficient buffer is checked against the header before anything is read.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/bevfusion_hip.h"

namespace bfjpeg_enc {

constexpr int kErrLen = 160;

// zigzag position -> natural (row-major) position
constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K, tables K.3 - K.6: the number of codes of each length 1 .. 16, then the symbols in code order
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

constexpr int kMaxBlockBits = 1664;  // 22 for the DC (11-bit code + 11) and 63 x 26 (16-bit code + 10), rounded up to whole words

// (code << 8) | length per symbol, 0 for a symbol without a code; table 0 codes luma, table 1 chroma
struct Tables {
  uint32_t dc[2][16];
  uint32_t ac[2][256];
};

constexpr Tables make_tables() {
  Tables t = {};
  for (int k = 0; k < 2; ++k) {
    uint32_t code = 0;
    int at = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < kDcBits[k][len - 1]; ++i) t.dc[k][kDcVals[at++]] = (code++ << 8) | (uint32_t)len;
      code <<= 1;
    }
    code = 0;
    at = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < kAcBits[k][len - 1]; ++i) t.ac[k][kAcVals[k][at++]] = (code++ << 8) | (uint32_t)len;
      code <<= 1;
    }
  }
  return t;
}

static constexpr Tables kTables = make_tables();

inline int fail(char *err, const char *msg) {
  if (err) snprintf(err, kErrLen, "jpeg encode: %s", msg);
  return BFHIP_E_INVALID;
}

// The geometry a header must have for sampling hs x vs; the quantisation tables are not looked at.
inline bool consistent(const bfhip_jpeg_header *h) {
  if (h->width < 1 || h->height < 1 || h->width > 65535 || h->height > 65535) return false;
  const int hs = h->hs[0], vs = h->vs[0];
  if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
  if (h->hs[1] != 1 || h->vs[1] != 1 || h->hs[2] != 1 || h->vs[2] != 1) return false;
  const int mx = (h->width + 8 * hs - 1) / (8 * hs), my = (h->height + 8 * vs - 1) / (8 * vs);
  if (h->mcus_x != mx || h->mcus_y != my) return false;
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    if (h->block_cols[c] != mx * h->hs[c] || h->block_rows[c] != my * h->vs[c] || h->coef_offset[c] != off) return false;
    off += (int64_t)h->block_cols[c] * h->block_rows[c] * 64;
  }
  return h->coef_bytes == off * 2;
}

struct Sink {
  uint8_t *out;
  size_t cap, n;  // n counts every byte, stored or not
  uint64_t acc;
  int cnt;
  int64_t stuffed;
  inline void put(uint8_t b) {
    if (n < cap) out[n] = b;
    ++n;
  }
  inline void bits(uint32_t code, int len) {  // len <= 26, cnt < 8 on entry
    acc = (acc << len) | code;
    cnt += len;
    while (cnt >= 8) {
      const uint8_t b = (uint8_t)(acc >> (cnt - 8));
      put(b);
      if (b == 0xFF) { put(0); ++stuffed; }
      cnt -= 8;
    }
  }
  inline void flush() {  // pads the last byte of an interval with 1-bits
    if (cnt) bits((1u << (8 - cnt)) - 1u, 8 - cnt);
    acc = 0;
  }
};

inline int category(int v) {
  unsigned a = (unsigned)(v < 0 ? -v : v);
  int s = 0;
  while (a) { ++s; a >>= 1; }
  return s;
}

// The scan and the EOI marker behind it.  restart_interval in MCUs, 0 = none.
inline int entropy_encode(const bfhip_jpeg_header *h, const int16_t *coef, size_t coef_bytes, int restart_interval, uint8_t *out,
                          size_t capacity, bfhip_jpeg_enc_stats *stats, char *err) {
  bfhip_jpeg_enc_stats local;
  if (!stats) stats = &local;
  memset(stats, 0, sizeof(*stats));
  if (!h || !coef || (!out && capacity)) return fail(err, "null argument");
  if (!consistent(h)) return fail(err, "the header's block counts do not fit its size and sampling");
  if ((uint64_t)h->coef_bytes > (uint64_t)coef_bytes) return fail(err, "coefficient buffer too small");
  if (restart_interval < 0 || restart_interval > 65535) return fail(err, "restart interval outside 0..65535");
  Sink s = {out, capacity, 0, 0, 0, 0};
  int pred[3] = {0, 0, 0};
  const long long mcus = (long long)h->mcus_x * h->mcus_y;
  int to_restart = restart_interval, next_rst = 0;
  for (long long m = 0; m < mcus; ++m) {
    if (restart_interval && to_restart == 0) {
      s.flush();
      s.put(0xFF);
      s.put((uint8_t)(0xD0 + next_rst));
      next_rst = (next_rst + 1) & 7;
      pred[0] = pred[1] = pred[2] = 0;
      to_restart = restart_interval;
    }
    --to_restart;
    const int my = (int)(m / h->mcus_x), mx = (int)(m % h->mcus_x);
    for (int c = 0; c < 3; ++c) {
      const int tb = c ? 1 : 0;
      for (int v = 0; v < h->vs[c]; ++v) {
        for (int u = 0; u < h->hs[c]; ++u) {
          const long long brow = (long long)my * h->vs[c] + v, bcol = (long long)mx * h->hs[c] + u;
          const int16_t *blk = coef + h->coef_offset[c] + (brow * h->block_cols[c] + bcol) * 64;
          const int diff = (int)blk[0] - pred[c];
          pred[c] = blk[0];
          int cat = category(diff);
          if (cat > 11) return fail(err, "a DC difference outside +-2047 has no Huffman code");
          if (cat > stats->max_dc_category) stats->max_dc_category = cat;
          uint32_t e = kTables.dc[tb][cat];
          s.bits(e >> 8, (int)(e & 255));
          if (cat) s.bits((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u), cat);
          int run = 0;
          for (int k = 1; k < 64; ++k) {
            const int x = blk[kNatural[k]];
            if (x == 0) { ++run; continue; }
            cat = category(x);
            if (cat > 10) return fail(err, "an AC coefficient outside +-1023 has no Huffman code");
            if (cat > stats->max_ac_category) stats->max_ac_category = cat;
            for (; run > 15; run -= 16) {
              e = kTables.ac[tb][0xF0];
              s.bits(e >> 8, (int)(e & 255));
              ++stats->zrl;
            }
            e = kTables.ac[tb][(run << 4) | cat];
            s.bits((e >> 8) << cat | ((uint32_t)(x < 0 ? x - 1 : x) & ((1u << cat) - 1u)), (int)(e & 255) + cat);
            run = 0;
          }
          if (run) {
            e = kTables.ac[tb][0];
            s.bits(e >> 8, (int)(e & 255));
            ++stats->eob;
          }
        }
      }
    }
  }
  s.flush();
  s.put(0xFF);
  s.put(0xD9);
  stats->bytes = (int64_t)s.n;
  stats->stuffed = s.stuffed;
  if (s.n > capacity) return fail(err, "output buffer too small");
  return BFHIP_OK;
}

}  // namespace bfjpeg_enc
