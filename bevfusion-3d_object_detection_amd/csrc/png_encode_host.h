// png_encode_host.h -- the PNG encoder's format in plain C++ with no HIP call: the row filter, the run tokens, the length-limited
// prefix code (package-merge) and the band-wise DEFLATE writer, so that a stand-alone program can run them under a sanitiser
// (tools/png_encode_host_check.cpp).  Included by csrc/png_encode.hip: the small functions marked BFPNG_HD are the very code the
// kernels run, and deflate_rle below defines the device stream byte for byte.  bevfusion_amd/png_encode.py states the same
// format in Python (huffman_lengths there IS the definition of the code lengths).
//
// The stream: 78 01, then one DEFLATE block per band of `band_bytes` input bytes, every band starting on a byte boundary.
//   tokens   within a band a maximal stretch of equal bytes is a literal, then matches of distance 1 and length min(r, 258)
//            while r >= 3 bytes remain, then 0-2 literals.  No other matches.
//   dynamic  BFINAL (last band only), BTYPE 10, HLIT 29, HDIST 0, HCLEN 15; the code-length code gives symbols 0-15 four bits
//            and 16-18 none, so a length L is written as the 4-bit code L (bit-reversed, as every Huffman code); 286 lengths of
//            the literal/length code; one distance length, 1 when the band has a match and 0 otherwise: kHeaderBits = 1222.  The
//            body, end-of-block, and -- unless it is the last band -- an empty stored block (000, pad, 00 00 FF FF).
//   stored   a band whose dynamic form is not smaller than n + 5 ceil(n / 65535) bytes goes out as stored blocks of at most
//            65535 bytes instead.
// Capacity: every band takes at most stored_bytes(n) bytes whichever form it has, so a stream is never longer than
//   capacity(n, band_bytes) = 2 + sum over the bands of stored_bytes(n_b); the Adler-32 trailer (4 bytes) is the caller's,
//   combined from the (A, B, n) triples the encoders leave per band.
// Every output byte goes through Sink::put, which counts always and stores only below the capacity.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/bevfusion_hip.h"

#if defined(__HIPCC__)
#define BFPNG_HD __host__ __device__
#else
#define BFPNG_HD
#endif

namespace bfpng {

constexpr int kErrLen = 160;
constexpr int kSymbols = 286;  // literals, end-of-block, 29 length codes
constexpr int kEob = 256;
constexpr int kMaxLen = 15;
constexpr int kMaxMatch = 258;
constexpr int kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
constexpr int kPrefixBits = 3 + 5 + 5 + 4 + 19 * 3;             // block header, HLIT, HDIST, HCLEN, the code-length code
constexpr int kHeaderBits = kPrefixBits + 4 * kSymbols + 4;    // 1222
constexpr long long kMaxBandBytes = 1ll << 26;                 // Adler partial sums and bit offsets stay inside 64 / 32 bits
constexpr long long kMaxBytes = (1ll << 31) - 1;
constexpr uint32_t kAdlerMod = 65521;
constexpr int kLevelWords = (2 * kSymbols + 31) / 32;
constexpr int kBandWords = 4;                                  // per band in the result: A, B, n, bytes | stored << 31
constexpr int kResultWords = 8;                                // per job: length lo, hi, flags, stored, dynamic, max len, bands, 0

BFPNG_HD inline long long stored_bytes(long long n) { return n + 5 * ((n + 65534) / 65535); }
BFPNG_HD inline long long band_count(long long n, long long band_bytes) { return (n + band_bytes - 1) / band_bytes; }

// the proved bound of a stream without its Adler-32 trailer
BFPNG_HD inline long long capacity(long long n, long long band_bytes) {
  const long long full = n / band_bytes, rest = n - full * band_bytes;
  return 2 + full * stored_bytes(band_bytes) + (rest ? stored_bytes(rest) : 0);
}

BFPNG_HD inline int filter_cost(int v) { return v < 128 ? v : 256 - v; }

// PNG filter `type` of byte x with left a, above b, above-left c (all raw)
BFPNG_HD inline int filter_byte(int type, int x, int a, int b, int c) {
  int p = 0;
  if (type == 1) p = a;
  else if (type == 2) p = b;
  else if (type == 3) p = (a + b) >> 1;
  else if (type == 4) {
    int pa = b - c, pb = a - c, pc = a + b - 2 * c;
    pa = pa < 0 ? -pa : pa; pb = pb < 0 ? -pb : pb; pc = pc < 0 ? -pc : pc;
    p = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return (x - p) & 255;
}

// a match length 3 .. 258 -> its symbol, the number of extra bits and their value (RFC 1951, 3.2.5)
BFPNG_HD inline void length_symbol(int len, int *sym, int *nextra, int *extra) {
  if (len == 258) { *sym = 285; *nextra = 0; *extra = 0; return; }
  const int v = len - 3;
  if (v < 8) { *sym = 257 + v; *nextra = 0; *extra = 0; return; }
  int top = 3;
  while (v >> (top + 1)) ++top;
  const int e = top - 2;
  *sym = 257 + 4 * (e + 1) + ((v >> e) & 3);
  *nextra = e;
  *extra = v & ((1 << e) - 1);
}

BFPNG_HD inline int length_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }

// A stretch of `run` equal bytes: one literal, q matches of 258, then a match of `rem` (rem >= 3) or `rem` literals
struct RunPlan { long long q; int rem; };
BFPNG_HD inline RunPlan plan_run(long long run) {
  RunPlan p;
  p.q = (run - 1) / kMaxMatch;
  p.rem = (int)((run - 1) - p.q * kMaxMatch);
  return p;
}

struct HuffScratch {
  uint64_t w[kSymbols];               // the used symbols' counts, ascending, ties by symbol index
  uint64_t level[2][2 * kSymbols];    // the list of this level and of the one before
  uint32_t leaf[kMaxLen][kLevelWords];  // bit i of level l: item i is a leaf (not a package)
  uint16_t sym[kSymbols];             // rank -> symbol
  int32_t a[kMaxLen];                 // leaves selected at level l
};

// Package-merge over n >= 2 sorted weights: list 0 holds the leaves; list l the leaves merged with the pairs of list l - 1 (a
// leaf before a package of the same weight), cut at 2 n - 2 items; the first 2 n - 2 items of the last list are selected, and
// a selected package selects its two items one level down.  a[l] = leaves selected at level l; the symbol of rank r gets as
// many bits as there are levels with r < a[l].
BFPNG_HD inline void package_merge(HuffScratch *s, int n, int max_len) {
  const int keep = 2 * n - 2;
  int before = 0;
  for (int l = 0; l < max_len; ++l) {
    uint64_t *cur = s->level[l & 1];
    const uint64_t *prev = s->level[(l & 1) ^ 1];
    for (int k = 0; k < kLevelWords; ++k) s->leaf[l][k] = 0;
    const int packages = before / 2;
    int i = 0, k = 0, m = 0;
    while (m < keep && (i < n || k < packages)) {
      bool take_leaf = i < n;
      uint64_t pw = 0;
      if (k < packages) {
        pw = prev[2 * k] + prev[2 * k + 1];
        take_leaf = i < n && s->w[i] <= pw;
      }
      if (take_leaf) {
        cur[m] = s->w[i++];
        s->leaf[l][m >> 5] |= 1u << (m & 31);
      } else {
        cur[m] = pw;
        ++k;
      }
      ++m;
    }
    before = m;
  }
  int take = keep;
  for (int l = max_len - 1; l >= 0; --l) {
    int leaves = 0;
    for (int i = 0; i < take; ++i) leaves += (s->leaf[l][i >> 5] >> (i & 31)) & 1;
    s->a[l] = leaves;
    take = 2 * (take - leaves);
  }
}

BFPNG_HD inline int rank_length(const HuffScratch *s, int rank, int max_len) {
  int len = 0;
  for (int l = 0; l < max_len; ++l) len += rank < s->a[l] ? 1 : 0;
  return len;
}

inline int fail(char *err, const char *msg) {
  if (err) snprintf(err, kErrLen, "png encode: %s", msg);
  return BFHIP_E_INVALID;
}

// lens[n_symbols] from hist[n_symbols]: 0 for an unused symbol, 1 for a single used one, package-merge otherwise
inline int huffman_lengths(const uint32_t *hist, int n_symbols, int max_len, uint8_t *lens, char *err) {
  if (!hist || !lens || n_symbols < 1 || n_symbols > kSymbols || max_len < 1 || max_len > kMaxLen)
    return fail(err, "huffman_lengths: 1..286 symbols and 1..15 bits");
  static thread_local HuffScratch s;
  int n = 0;
  for (int t = 0; t < n_symbols; ++t) {
    lens[t] = 0;
    if (!hist[t]) continue;
    int at = n++;
    for (; at > 0 && s.w[at - 1] > hist[t]; --at) { s.w[at] = s.w[at - 1]; s.sym[at] = s.sym[at - 1]; }  // stable: ties by index
    s.w[at] = hist[t];
    s.sym[at] = (uint16_t)t;
  }
  if (n == 0) return BFHIP_OK;
  if (n == 1) { lens[s.sym[0]] = 1; return BFHIP_OK; }
  if ((1 << max_len) < n) return fail(err, "huffman_lengths: more symbols than codes of that length");
  package_merge(&s, n, max_len);
  for (int r = 0; r < n; ++r) lens[s.sym[r]] = (uint8_t)rank_length(&s, r, max_len);
  return BFHIP_OK;
}

BFPNG_HD inline uint32_t reverse_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

// canonical codes (RFC 1951, 3.2.2), bit-reversed for the LSB-first writer: codes[s] = reversed << 8 | length
inline void canonical_codes(const uint8_t *lens, int n_symbols, uint32_t *codes) {
  uint32_t count[kMaxLen + 2] = {0}, next[kMaxLen + 2] = {0};
  for (int t = 0; t < n_symbols; ++t) ++count[lens[t]];
  count[0] = 0;
  uint32_t code = 0;
  for (int b = 1; b <= kMaxLen; ++b) { code = (code + count[b - 1]) << 1; next[b] = code; }
  for (int t = 0; t < n_symbols; ++t) codes[t] = lens[t] ? (reverse_bits(next[lens[t]]++, lens[t]) << 8) | lens[t] : 0;
}

struct Sink {
  uint8_t *out;
  size_t capacity, at;
  uint64_t acc;
  int n;
  void put(uint8_t b) { if (at < capacity) out[at] = b; ++at; }
  void bits(uint32_t v, int len) {
    acc |= (uint64_t)v << n;
    n += len;
    while (n >= 8) { put((uint8_t)acc); acc >>= 8; n -= 8; }
  }
  void align() { if (n) { put((uint8_t)acc); acc = 0; n = 0; } }
};

// the row filter: rgb uint8 [height, width, 3] -> out [height, 1 + 3 width], the type with the least sum of filter_cost (the
// lowest type on a tie) in front of every row; the row above the first and the bytes left of the first pixel are zero
inline int filter_rows(const uint8_t *rgb, int width, int height, uint8_t *out, size_t out_bytes, char *err) {
  if (!rgb || !out || width < 1 || height < 1) return fail(err, "filter_rows: null or empty image");
  const size_t rb = 3 * (size_t)width;
  if (out_bytes < (size_t)height * (rb + 1)) return fail(err, "filter_rows: the output holds fewer than height (1 + 3 width) bytes");
  for (int y = 0; y < height; ++y) {
    const uint8_t *cur = rgb + (size_t)y * rb, *up = y ? cur - rb : nullptr;
    uint64_t cost[5] = {0, 0, 0, 0, 0};
    for (size_t i = 0; i < rb; ++i) {
      const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = up ? up[i] : 0, c = up && i >= 3 ? up[i - 3] : 0;
      for (int t = 0; t < 5; ++t) cost[t] += (uint64_t)filter_cost(filter_byte(t, x, a, b, c));
    }
    int type = 0;
    for (int t = 1; t < 5; ++t) if (cost[t] < cost[type]) type = t;
    uint8_t *dst = out + (size_t)y * (rb + 1);
    dst[0] = (uint8_t)type;
    for (size_t i = 0; i < rb; ++i)
      dst[1 + i] = (uint8_t)filter_byte(type, cur[i], i >= 3 ? cur[i - 3] : 0, up ? up[i] : 0, up && i >= 3 ? up[i - 3] : 0);
  }
  return BFHIP_OK;
}

// data[0 .. n) -> out[0 .. capacity): 78 01 and the bands, without the Adler-32 trailer.  bands (may be null): kBandWords
// words per band, band_slots of them: Adler A and B of the band alone, its length, its bytes in the stream | stored << 31.
// BFHIP_E_INVALID with nothing written at or past `capacity` when the stream is longer (stats->bytes holds the length).
inline int deflate_rle(const uint8_t *data, size_t n, size_t band_bytes, uint8_t *out, size_t cap, uint32_t *bands, size_t band_slots,
                       bfhip_png_stats *stats, char *err) {
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!data || (!out && cap) || n < 1 || (long long)n > kMaxBytes || band_bytes < 1 || (long long)band_bytes > kMaxBandBytes)
    return fail(err, "deflate_rle: 1 .. 2^31 - 1 bytes in bands of 1 .. 2^26");
  const size_t n_bands = (size_t)band_count((long long)n, (long long)band_bytes);
  if (bands && band_slots < n_bands) return fail(err, "deflate_rle: fewer band slots than bands");
  Sink s = {out, cap, 0, 0, 0};
  s.put(0x78);
  s.put(0x01);
  static thread_local uint32_t hist[kSymbols], codes[kSymbols];
  uint8_t lens[kSymbols];
  int64_t stored_bands = 0, dynamic_bands = 0, tokens = 0;
  int max_len = 0;
  for (size_t bi = 0; bi < n_bands; ++bi) {
    const uint8_t *d = data + bi * band_bytes;
    const size_t nb = bi + 1 == n_bands ? n - bi * band_bytes : band_bytes;
    const bool final = bi + 1 == n_bands;
    const size_t begin = s.at;
    memset(hist, 0, sizeof(hist));
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < nb; ++i) { a += d[i]; if (a >= kAdlerMod) a -= kAdlerMod; b += a; if (b >= kAdlerMod) b -= kAdlerMod; }
    uint64_t matches = 0;
    for (size_t i = 0; i < nb;) {
      size_t e = i + 1;
      while (e < nb && d[e] == d[i]) ++e;
      const RunPlan p = plan_run((long long)(e - i));
      hist[d[i]] += 1 + (p.rem < 3 ? p.rem : 0);
      hist[285] += (uint32_t)p.q;
      matches += (uint64_t)p.q;
      if (p.rem >= 3) {
        int sym, ne, ex;
        length_symbol(p.rem, &sym, &ne, &ex);
        ++hist[sym];
        ++matches;
      }
      i = e;
    }
    hist[kEob] = 1;
    int rc = huffman_lengths(hist, kSymbols, kMaxLen, lens, err);
    if (rc) return rc;
    uint64_t bits = kHeaderBits + matches;
    for (int t = 0; t < kSymbols; ++t) {
      bits += (uint64_t)hist[t] * (uint64_t)(lens[t] + (t > kEob ? length_extra_bits(t) : 0));
      tokens += hist[t];
      if (hist[t] && lens[t] > max_len) max_len = lens[t];
    }
    const uint64_t dyn_bytes = final ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
    const bool stored = dyn_bytes >= (uint64_t)stored_bytes((long long)nb);
    if (stored) {
      ++stored_bands;
      for (size_t at = 0; at < nb; at += 65535) {
        const size_t len = nb - at < 65535 ? nb - at : 65535;
        s.put(final && at + len == nb ? 1 : 0);
        s.put((uint8_t)len); s.put((uint8_t)(len >> 8)); s.put((uint8_t)~len); s.put((uint8_t)(~len >> 8));
        for (size_t i = 0; i < len; ++i) s.put(d[at + i]);
      }
    } else {
      ++dynamic_bands;
      canonical_codes(lens, kSymbols, codes);
      s.bits(final ? 1 : 0, 1);
      s.bits(2, 2);
      s.bits(29, 5);
      s.bits(0, 5);
      s.bits(15, 4);
      for (int k = 0; k < 19; ++k) s.bits(kClOrder[k] < 16 ? 4 : 0, 3);
      for (int t = 0; t < kSymbols; ++t) s.bits(reverse_bits(lens[t], 4), 4);
      s.bits(reverse_bits(matches ? 1 : 0, 4), 4);
      for (size_t i = 0; i < nb;) {
        size_t e = i + 1;
        while (e < nb && d[e] == d[i]) ++e;
        const RunPlan p = plan_run((long long)(e - i));
        const uint32_t lit = codes[d[i]];
        s.bits(lit >> 8, (int)(lit & 255));
        for (long long k = 0; k < p.q; ++k) { s.bits(codes[285] >> 8, (int)(codes[285] & 255)); s.bits(0, 1); }
        if (p.rem >= 3) {
          int sym, ne, ex;
          length_symbol(p.rem, &sym, &ne, &ex);
          s.bits(codes[sym] >> 8, (int)(codes[sym] & 255));
          if (ne) s.bits((uint32_t)ex, ne);
          s.bits(0, 1);
        } else {
          for (int k = 0; k < p.rem; ++k) s.bits(lit >> 8, (int)(lit & 255));
        }
        i = e;
      }
      s.bits(codes[kEob] >> 8, (int)(codes[kEob] & 255));
      if (!final) {
        s.bits(0, 3);
        s.align();
        s.put(0); s.put(0); s.put(0xFF); s.put(0xFF);
      } else {
        s.align();
      }
    }
    if (bands) {
      uint32_t *r = bands + bi * kBandWords;
      r[0] = a; r[1] = b; r[2] = (uint32_t)nb; r[3] = (uint32_t)(s.at - begin) | (stored ? 0x80000000u : 0u);
    }
  }
  if (stats) {
    stats->bytes = (int64_t)s.at;
    stats->bands = (int64_t)n_bands;
    stats->stored_bands = stored_bands;
    stats->dynamic_bands = dynamic_bands;
    stats->tokens = tokens;
    stats->max_code_length = max_len;
    stats->overflow = s.at > cap ? 1 : 0;
  }
  if (s.at > cap) return fail(err, "deflate_rle: the stream is longer than the capacity");
  return BFHIP_OK;
}

}  // namespace bfpng
