// jpeg_host.h -- the host half of the JPEG decoder: marker parsing and the Huffman (entropy) stage of baseline sequential
// streams, in plain C++ with no HIP call, so that a loader's worker can run it without ever opening the device and a
// stand-alone program can run it under a sanitiser (tools/jpeg_host_check.cpp).  Included by csrc/jpeg.hip.
//
// Both entry points take untrusted bytes: every read goes through a length check against `n`, every coefficient write lands
// inside the block the MCU loop addresses, and the buffer is checked against the header's coef_bytes before anything is written.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/bevfusion_hip.h"

namespace bfjpeg {

constexpr int kErrLen = 160;

// zigzag position -> natural (row-major) position; 16 spare entries as libjpeg keeps, although k is checked before use
static const uint8_t kNatural[64 + 16] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
    63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

constexpr int kLookBits = 9;

struct Huff {
  bool present;
  uint8_t vals[256];
  int32_t maxcode[18];  // largest code of each length, -1 when none; [17] is a sentinel that ends every search
  int32_t valoff[17];   // vals index of the first code of the length minus that code
  uint16_t look[1 << kLookBits];  // (length << 8) | symbol for codes of up to kLookBits bits, 0 when longer
};

struct Stream {
  Huff dc[4], ac[4];
  bool quant_present[4];
  bool quant16[4];
  uint16_t quant[4][64];  // natural order
  int tq[3], td[3], ta[3];
  size_t scan_begin;  // first entropy-coded byte
  int restart_interval;
};

inline int fail(char *err, const char *msg) {
  if (err) snprintf(err, kErrLen, "jpeg: %s", msg);
  return BFHIP_E_INVALID;
}

inline bool build_huff(Huff *h, const uint8_t *bits /* [1..16] */, const uint8_t *vals, int nvals) {
  memset(h, 0, sizeof(*h));
  memcpy(h->vals, vals, (size_t)nvals);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int cnt = bits[len];
    h->valoff[len] = k - code;
    if (cnt) {
      if (code + cnt > (1 << len)) return false;  // more codes than the length holds
      if (len <= kLookBits) {
        for (int i = 0; i < cnt; ++i) {
          const int first = (code + i) << (kLookBits - len), span = 1 << (kLookBits - len);
          for (int j = 0; j < span; ++j) h->look[first + j] = (uint16_t)((len << 8) | vals[k + i]);
        }
      }
      code += cnt;
      k += cnt;
      h->maxcode[len] = code - 1;
    } else {
      h->maxcode[len] = -1;
    }
    code <<= 1;
  }
  h->maxcode[17] = 0x7fffffff;
  h->present = true;
  return true;
}

// EXIF (APP1) payload: 1 when IFD0 holds the orientation tag 0x0112, 0 when it does not, 1 as well when the TIFF structure
// cannot be followed (the fused path then leaves the file to the host decoder)
inline int exif_has_orientation(const uint8_t *p, size_t n) {
  if (n < 14 || memcmp(p, "Exif\0\0", 6) != 0) return 0;
  const uint8_t *t = p + 6;
  const size_t tn = n - 6;
  bool le;
  if (t[0] == 'I' && t[1] == 'I') le = true;
  else if (t[0] == 'M' && t[1] == 'M') le = false;
  else return 1;
  auto u16 = [&](size_t o) -> uint32_t { return le ? (uint32_t)(t[o] | (t[o + 1] << 8)) : (uint32_t)((t[o] << 8) | t[o + 1]); };
  auto u32 = [&](size_t o) -> uint32_t {
    return le ? ((uint32_t)t[o] | ((uint32_t)t[o + 1] << 8) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24))
              : (((uint32_t)t[o] << 24) | ((uint32_t)t[o + 1] << 16) | ((uint32_t)t[o + 2] << 8) | (uint32_t)t[o + 3]);
  };
  const size_t ifd = u32(4);
  if (ifd > tn || tn - ifd < 2) return 1;
  const size_t count = u16(ifd);
  for (size_t i = 0; i < count; ++i) {
    const size_t e = ifd + 2 + 12 * i;
    if (e > tn || tn - e < 12) return 1;
    if (u16(e) == 0x0112) return 1;
  }
  return 0;
}

// Markers up to and including the first SOS.  Fills the public header (geometry, sampling, quantisation tables, the
// `supported` verdict) and, when `st` is given, what the entropy stage needs.  0, or BFHIP_E_INVALID for a malformed stream.
inline int parse(const uint8_t *d, size_t n, bfhip_jpeg_header *h, Stream *st, char *err) {
  memset(h, 0, sizeof(*h));
  Stream local;
  if (!st) st = &local;
  memset(st, 0, sizeof(*st));
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(err, "no SOI marker");
  size_t p = 2;
  int reason = 0;
  bool have_sof = false;
  int comp_id[4] = {0, 0, 0, 0};
  bool saw_jfif = false;
  int adobe_transform = -1;
  auto flag = [&](int r) { if (!reason) reason = r; };
  for (;;) {
    if (p >= n || d[p] != 0xFF) return fail(err, "marker expected");
    while (p < n && d[p] == 0xFF) ++p;  // fill bytes
    if (p >= n) return fail(err, "truncated at a marker");
    const int m = d[p++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // no length
    if (m == 0xD9) return fail(err, "EOI before a scan");
    if (n - p < 2) return fail(err, "truncated segment length");
    const size_t len = ((size_t)d[p] << 8) | d[p + 1];
    if (len < 2 || len > n - p) return fail(err, "segment runs past the end");
    const uint8_t *s = d + p + 2;
    const size_t sn = len - 2;
    if (m == 0xDB) {  // DQT
      size_t o = 0;
      while (o < sn) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (tq > 3 || pq > 1) return fail(err, "bad DQT");
        const size_t need = pq ? 128 : 64;
        if (sn - o - 1 < need) return fail(err, "short DQT");
        for (int i = 0; i < 64; ++i) {
          const uint32_t v = pq ? (((uint32_t)s[o + 1 + 2 * i] << 8) | s[o + 2 + 2 * i]) : s[o + 1 + i];
          st->quant[tq][kNatural[i]] = (uint16_t)v;
        }
        st->quant_present[tq] = true;
        st->quant16[tq] = pq != 0;
        o += 1 + need;
      }
    } else if (m == 0xC4) {  // DHT
      size_t o = 0;
      while (o < sn) {
        if (sn - o < 17) return fail(err, "short DHT");
        const int tc = s[o] >> 4, th = s[o] & 15;
        if (tc > 1 || th > 3) return fail(err, "bad DHT");
        uint8_t bits[17];
        bits[0] = 0;
        int total = 0;
        for (int i = 1; i <= 16; ++i) total += (bits[i] = s[o + i]);
        if (total > 256 || (size_t)total > sn - o - 17) return fail(err, "bad DHT counts");
        if (!build_huff(tc ? &st->ac[th] : &st->dc[th], bits, s + o + 17, total)) return fail(err, "bad DHT code lengths");
        o += 17 + (size_t)total;
      }
    } else if (m == 0xDD) {  // DRI
      if (sn < 2) return fail(err, "short DRI");
      st->restart_interval = (s[0] << 8) | s[1];
    } else if (m == 0xE0) {
      if (sn >= 5 && memcmp(s, "JFIF\0", 5) == 0) saw_jfif = true;
    } else if (m == 0xEE) {
      if (sn >= 12 && memcmp(s, "Adobe", 5) == 0) adobe_transform = s[11];
    } else if (m == 0xE1) {
      if (exif_has_orientation(s, sn)) flag(BFHIP_JPEG_R_EXIF_ORIENTATION);
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {  // SOFn (0xC4 handled above)
      if (have_sof) return fail(err, "two frame headers");
      if (sn < 6) return fail(err, "short SOF");
      have_sof = true;
      if (m == 0xC2) flag(BFHIP_JPEG_R_PROGRESSIVE);
      else if (m >= 0xC9) flag(BFHIP_JPEG_R_ARITHMETIC);
      else if (m != 0xC0) flag(BFHIP_JPEG_R_NOT_BASELINE);
      if (s[0] != 8) flag(BFHIP_JPEG_R_PRECISION);
      h->height = (s[1] << 8) | s[2];
      h->width = (s[3] << 8) | s[4];
      h->ncomp = s[5];
      if (h->width <= 0 || h->height <= 0) return fail(err, "empty image");
      if (h->ncomp < 1 || h->ncomp > 4 || sn < 6 + 3 * (size_t)h->ncomp) return fail(err, "bad component count");
      if (h->ncomp != 3) flag(BFHIP_JPEG_R_COMPONENTS);
      for (int c = 0; c < h->ncomp && c < 3; ++c) {
        comp_id[c] = s[6 + 3 * c];
        h->hs[c] = s[7 + 3 * c] >> 4;
        h->vs[c] = s[7 + 3 * c] & 15;
        st->tq[c] = s[8 + 3 * c];
        if (h->hs[c] < 1 || h->hs[c] > 4 || h->vs[c] < 1 || h->vs[c] > 4 || st->tq[c] > 3) return fail(err, "bad SOF component");
      }
      if (h->ncomp == 3 && !(h->hs[0] <= 2 && h->vs[0] <= 2 && h->hs[1] == 1 && h->vs[1] == 1 && h->hs[2] == 1 && h->vs[2] == 1))
        flag(BFHIP_JPEG_R_SAMPLING);
    } else if (m == 0xDA) {  // SOS
      if (!have_sof) return fail(err, "scan before the frame header");
      if (sn < 1) return fail(err, "short SOS");
      const int ns = s[0];
      if (ns < 1 || ns > 4 || sn < 1 + 2 * (size_t)ns + 3) return fail(err, "bad SOS");
      if (ns != h->ncomp) flag(BFHIP_JPEG_R_MULTI_SCAN);
      // libjpeg's guess of the colour space: JFIF means YCbCr, then Adobe's transform flag, then the component ids
      if (!saw_jfif && (adobe_transform >= 0 ? adobe_transform != 1 : (comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')))
        flag(BFHIP_JPEG_R_COLOUR_SPACE);
      if (!reason) {
        for (int c = 0; c < 3; ++c) {
          if (s[1 + 2 * c] != comp_id[c]) return fail(err, "scan components out of order");
          st->td[c] = s[2 + 2 * c] >> 4;
          st->ta[c] = s[2 + 2 * c] & 15;
          if (st->td[c] > 3 || st->ta[c] > 3 || !st->dc[st->td[c]].present || !st->ac[st->ta[c]].present)
            return fail(err, "scan names a Huffman table the file does not define");
          if (!st->quant_present[st->tq[c]]) return fail(err, "component names a quantisation table the file does not define");
          if (st->quant16[st->tq[c]]) flag(BFHIP_JPEG_R_QUANT16);
        }
        if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return fail(err, "bad spectral selection");
      }
      st->scan_begin = p + len;
      break;
    }
    p += len;
  }
  h->reason = reason;
  h->supported = reason == 0;
  h->restart_interval = st->restart_interval;
  if (reason) return BFHIP_OK;
  h->mcus_x = (h->width + 8 * h->hs[0] - 1) / (8 * h->hs[0]);
  h->mcus_y = (h->height + 8 * h->vs[0] - 1) / (8 * h->vs[0]);
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    h->block_cols[c] = h->mcus_x * h->hs[c];
    h->block_rows[c] = h->mcus_y * h->vs[c];
    h->coef_offset[c] = off;
    off += (int64_t)h->block_cols[c] * h->block_rows[c] * 64;
    memcpy(h->quant[c], st->quant[st->tq[c]], sizeof(h->quant[c]));
  }
  h->coef_bytes = off * 2;
  return BFHIP_OK;
}

// The bit reader of the entropy-coded segment: un-stuffs FF 00, stops at any other marker (or the end of the buffer) and
// feeds zero bits from there on, counting on `dry` that it did.
struct Bits {
  const uint8_t *d;
  size_t p, n;
  uint64_t acc;
  int cnt;
  bool dry;     // a marker or the end was reached: zero bits from here
  bool starved; // zero bits were consumed

  inline void fill() {
    while (cnt <= 56) {
      uint32_t b = 0;
      if (!dry) {
        if (p >= n) dry = true;
        else {
          b = d[p];
          if (b == 0xFF) {
            size_t q = p + 1;
            while (q < n && d[q] == 0xFF) ++q;  // FF FF ..: fill bytes before a marker
            if (q < n && d[q] == 0x00 && q == p + 1) p += 2;
            else { dry = true; b = 0; }  // a marker (left in place) or the end
          } else ++p;
        }
      }
      acc = (acc << 8) | b;
      cnt += 8;
      if (dry) pending_zero += 8;
    }
  }
  int pending_zero;  // zero bits sitting in acc
  inline uint32_t peek(int k) { return (uint32_t)(acc >> (cnt - k)) & ((1u << k) - 1u); }
  inline void drop(int k) {
    cnt -= k;
    if (cnt < pending_zero) { starved = true; pending_zero = cnt; }
  }
  inline void reset() { acc = 0; cnt = 0; pending_zero = 0; starved = false; }
};

inline int decode_symbol(Bits *b, const Huff *h) {
  if (b->cnt < 16) b->fill();
  const uint32_t look = h->look[b->peek(kLookBits)];
  if (look) { b->drop((int)(look >> 8)); return (int)(look & 255); }
  int len = kLookBits + 1;
  int32_t code = (int32_t)b->peek(len);
  while (code > h->maxcode[len]) { ++len; code = len <= 16 ? (int32_t)b->peek(len) : 0; }
  if (len > 16) return -1;
  b->drop(len);
  const int idx = code + h->valoff[len];
  return (idx >= 0 && idx < 256) ? h->vals[idx] : -1;
}

inline int receive_extend(Bits *b, int s) {
  if (b->cnt < s) b->fill();
  const int v = (int)b->peek(s);
  b->drop(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// Finds the next marker at or after b->p (a marker the reader stopped at is still there): its code, or -1 at the end.
inline int next_marker(Bits *b) {
  size_t p = b->p;
  while (p < b->n) {
    if (b->d[p] != 0xFF) { ++p; continue; }
    while (p < b->n && b->d[p] == 0xFF) ++p;
    if (p >= b->n) break;
    if (b->d[p] == 0x00) { ++p; continue; }
    b->p = p + 1;
    return b->d[p];
  }
  b->p = b->n;
  return -1;
}

// Entropy stage: per component [block_rows, block_cols, 64] int16 coefficients in natural order, DC prediction undone, not
// dequantised.  A stream that ends early (EOI or the end of the bytes inside the scan) leaves the remaining blocks zero, the
// MCU in which it ended decoded from zero bits, as libjpeg does.  0, or BFHIP_E_INVALID.
inline int entropy_decode(const uint8_t *d, size_t n, const bfhip_jpeg_header *want, int16_t *coef, size_t coef_bytes, char *err) {
  bfhip_jpeg_header h;
  Stream st;
  const int rc = parse(d, n, &h, &st, err);
  if (rc) return rc;
  if (!h.supported) return fail(err, "stream not supported by the fused decoder");
  if (!want || !coef) return fail(err, "null argument");
  if (want->width != h.width || want->height != h.height || want->coef_bytes != h.coef_bytes ||
      memcmp(want->hs, h.hs, sizeof(h.hs)) != 0 || memcmp(want->vs, h.vs, sizeof(h.vs)) != 0)
    return fail(err, "header does not belong to these bytes");
  if ((uint64_t)h.coef_bytes > (uint64_t)coef_bytes) return fail(err, "coefficient buffer too small");
  memset(coef, 0, (size_t)h.coef_bytes);

  Bits b;
  b.d = d; b.p = st.scan_begin; b.n = n; b.dry = false;
  b.reset();
  int pred[3] = {0, 0, 0};
  const long long mcus = (long long)h.mcus_x * h.mcus_y;
  int to_restart = st.restart_interval;
  bool insufficient = false;
  for (long long m = 0; m < mcus; ++m) {
    if (st.restart_interval && to_restart == 0) {
      b.reset();
      b.dry = false;
      const int mk = next_marker(&b);
      if (mk >= 0xD0 && mk <= 0xD7) {
        insufficient = false;
      } else {
        b.dry = true;  // EOI or the end: nothing more to decode
        b.p = n;
        insufficient = true;
      }
      pred[0] = pred[1] = pred[2] = 0;
      to_restart = st.restart_interval;
    }
    --to_restart;
    if (insufficient) continue;
    const int my = (int)(m / h.mcus_x), mx = (int)(m % h.mcus_x);
    for (int c = 0; c < 3; ++c) {
      const Huff *dc = &st.dc[st.td[c]], *ac = &st.ac[st.ta[c]];
      for (int v = 0; v < h.vs[c]; ++v) {
        for (int u = 0; u < h.hs[c]; ++u) {
          const long long brow = (long long)my * h.vs[c] + v, bcol = (long long)mx * h.hs[c] + u;
          int16_t *blk = coef + h.coef_offset[c] + (brow * h.block_cols[c] + bcol) * 64;
          int s = decode_symbol(&b, dc);
          if (s < 0 || s > 11) return fail(err, "bad DC code");
          if (s) pred[c] = (int)((uint32_t)pred[c] + (uint32_t)receive_extend(&b, s));  // wraps on a corrupt stream
          blk[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            const int rs = decode_symbol(&b, ac);
            if (rs < 0) return fail(err, "bad AC code");
            const int r = rs >> 4;
            s = rs & 15;
            if (s) {
              k += r;
              if (k > 63) return fail(err, "AC run past the block");
              if (s > 10) return fail(err, "bad AC size");
              blk[kNatural[k]] = (int16_t)receive_extend(&b, s);
              ++k;
            } else {
              if (r != 15) break;  // EOB
              k += 16;
            }
          }
        }
      }
    }
    if (b.starved) insufficient = true;  // the data ended inside this MCU: the rest stays zero
  }
  return BFHIP_OK;
}

}  // namespace bfjpeg
