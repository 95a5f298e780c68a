// text_parse.h -- the text event line `t x y p[ label]` read back (ae_text_output.py:86-101 inverted), for host and device: the
// mirror image of text_format.h.
//
// A line (without its '\n'; one '\r' at its end is dropped; blanks are ' ' and '\t'):
//   empty, only blanks, or first non-blank byte '#'   -> LINE_SKIP
//   t x y p        fields separated by one or more blanks, blanks allowed before the first and after the last
//   t x y p label
//     t      [+-]? (digits [. digits*]? | . digits) ([eE] [+-]? digits)?      -- no inf, nan, hex or underscores
//     x, y   [+-]? digits, |v| < 2^24 (exact in float32)
//     p      0 or 1 -> -1.0 / +1.0
//     label  0 or 1; with want_labels the fifth field is required, without it a fifth field is checked and ignored
//   anything else                                     -> LINE_BAD
//
// The time stamp is float32(float64 nearest the decimal, ties to even) -- np.float32(float(s)), two roundings -- computed with
// exact integer arithmetic: the first 19 significant digits as a 64-bit integer w and a decimal exponent e10 (value = w 10^e10);
// for e10 >= 0 the product w 5^e10 (at most 64 + 144 bits, the table text_format.h scales by), for e10 < 0 the quotient
// floor((w << S) / 5^-e10) with 63 or 64 significant bits and whether a remainder was left (long division by 5^13 at a time on
// 32-bit limbs).  The top 64 bits and "anything below" decide the float64, its 53 bits decide the float32; both roundings are
// done on integers, so host and device agree and no denormal mode matters.
//
// EXACTLY DECIDED: every decimal with at most 19 significant digits -- leading zeros, and zeros after the 19th digit, do not
// count -- and -62 <= e10 <= 62, e10 being the power of ten of the last kept digit; and every zero.  That covers the shortest
// repr of the float64 of every finite float32 (at most 17 digits, e10 >= -61: what the text sink writes) and fixed notation with
// up to 19 digits.  Anything else -- a nonzero digit after the 19th, e10 outside the table -- is LINE_ROW_FLAGGED: the row is
// emitted with a best-effort t (the digits truncated, the exponent clamped) and the caller parses that line's t again.
#pragma once
#include "text_format.h"

namespace v2e_tp {

enum { LINE_SKIP = 0, LINE_ROW = 1, LINE_ROW_FLAGGED = 2, LINE_BAD = 3 };

constexpr int MAX_DIGITS = 19;       // 10^19 < 2^64
constexpr int MAX_E10 = V2E_POW5_MAX; // the power-of-five table's reach, both ways

struct Row {
    float t, x, y, p;
    int label; // 0 / 1, or -1: the line has no fifth field
};

V2E_TF_HD bool is_blank(char c) { return c == ' ' || c == '\t'; }
V2E_TF_HD bool is_digit(char c) { return (unsigned)(c - '0') < 10u; }

// the float32 nearest (ties to even) to the float64 mant * 2^(E - 52), 2^52 <= mant < 2^53: its bits, sign clear
V2E_TF_HD uint32_t f64_to_f32_bits(uint64_t mant, int E)
{
    if (E >= -126) {
        uint64_t m = mant >> 29;
        const uint64_t rb = (mant >> 28) & 1u, st = mant & ((1ull << 28) - 1ull);
        if (rb && (st || (m & 1u))) ++m;
        if (m == (1ull << 24)) { m >>= 1; ++E; }
        if (E > 127) return 0x7F800000u;
        return ((uint32_t)(E + 127) << 23) | ((uint32_t)m & 0x7FFFFFu);
    }
    const int shift = 29 + (-126 - E); // a float32 subnormal: units of 2^-149
    if (shift > 54) return 0u;          // below half the smallest subnormal
    uint64_t m = mant >> shift;
    const uint64_t rb = (mant >> (shift - 1)) & 1u, st = mant & ((1ull << (shift - 1)) - 1ull);
    if (rb && (st || (m & 1u))) ++m;
    return (uint32_t)m; // 2^23 is the smallest normal's encoding
}

// float32(float64(T * 2^(E - 63) [+ something below one unit of T when sticky])), T's top bit set: its bits, sign clear
V2E_TF_HD uint32_t round_twice(uint64_t T, bool sticky, int E)
{
    uint64_t mant = T >> 11;
    const uint64_t rb = (T >> 10) & 1u;
    const bool st = sticky || (T & 0x3FFu);
    if (rb && (st || (mant & 1u))) ++mant;
    if (mant == (1ull << 53)) { mant >>= 1; ++E; }
    return f64_to_f32_bits(mant, E); // |E| < 300: a normal float64
}

// w * 10^e10 for w != 0 and |e10| <= MAX_E10; truncated: digits were dropped after w (the result is then a best effort)
V2E_TF_HD uint32_t decimal_to_f32_bits(uint64_t w, int e10, bool truncated)
{
    if (e10 >= 0) { // w * 5^e10 * 2^e10
        const unsigned long long *f = V2E_POW5[e10];
        uint64_t P[4];
        const uint64_t lo0 = w * f[0], hi0 = v2e_tf::mulhi64(w, f[0]);
        const uint64_t lo1 = w * f[1], hi1 = v2e_tf::mulhi64(w, f[1]);
        const uint64_t lo2 = w * f[2], hi2 = v2e_tf::mulhi64(w, f[2]);
        P[0] = lo0;
        P[1] = hi0 + lo1;
        const uint64_t c = P[1] < lo1;
        P[2] = hi1 + lo2;
        uint64_t c2 = P[2] < lo2;
        P[2] += c;
        c2 += P[2] < c;
        P[3] = hi2 + c2;
        int h = 3;
        while (h > 0 && P[h] == 0) --h;
        const int lz = __builtin_clzll(P[h]);
        uint64_t T = P[h] << lz;
        bool sticky = truncated;
        if (h > 0) {
            if (lz) T |= P[h - 1] >> (64 - lz);
            sticky = sticky || (uint64_t)(P[h - 1] << lz) != 0;
            for (int k = 0; k + 1 < h; ++k) sticky = sticky || P[k] != 0;
        }
        return round_twice(T, sticky, 64 * (h + 1) - lz - 1 + e10);
    }
    // e10 < 0: floor((w << S) / 5^p) * 2^(-S - p), S such that the quotient has 63 or 64 bits
    const int p = -e10;
    const unsigned long long *f = V2E_POW5[p];
    const int b5 = f[2] ? 192 - __builtin_clzll(f[2]) : (f[1] ? 128 - __builtin_clzll(f[1]) : 64 - __builtin_clzll(f[0]));
    const int S = 63 + b5 - (64 - __builtin_clzll(w)); // 2 <= S <= 207; the numerator has 63 + b5 <= 208 bits
    uint32_t n[10];
    for (int k = 0; k < 10; ++k) n[k] = 0;
    {
        const int li = S >> 5, b = S & 31;
        const uint64_t lo = w << b, hi = b ? (w >> (64 - b)) : 0;
        n[li] = (uint32_t)lo; n[li + 1] = (uint32_t)(lo >> 32); n[li + 2] = (uint32_t)hi; // li + 2 <= 8
    }
    bool sticky = truncated;
    int left = p;
    while (left > 0) {
        const int step = left > 13 ? 13 : left;
        const uint32_t d = (uint32_t)V2E_POW5[step][0]; // 5^13 < 2^32
        uint64_t rr = 0;
        for (int k = 6; k >= 0; --k) { // 7 limbs hold 208 bits
            const uint64_t cur = (rr << 32) | n[k];
            n[k] = (uint32_t)(cur / d);
            rr = cur % d;
        }
        sticky = sticky || rr != 0; // x = (x2 d2 + r2) d1 + r1: the remainder of x / (d1 d2) is zero iff r1 and r2 are
        left -= step;
    }
    const uint64_t Q = ((uint64_t)n[1] << 32) | n[0]; // 2^62 < Q < 2^64
    const int lz = __builtin_clzll(Q);
    return round_twice(Q << lz, sticky, 63 - lz - S - p);
}

// the time stamp field at s[i ..]: advances i past it.  false: not a number of the grammar.  flagged: outside the exactly
// decided domain (bits then hold the best effort).
V2E_TF_HD bool parse_time(const char *s, int64_t &i, int64_t len, uint32_t &bits, bool &flagged)
{
    uint32_t sign = 0;
    if (i < len && (s[i] == '+' || s[i] == '-')) { sign = s[i] == '-' ? 0x80000000u : 0u; ++i; }
    uint64_t w = 0;
    int64_t e10 = 0; // (a line is shorter than 2^62 bytes)
    int nd = 0;
    bool any = false, dropped = false;
    for (; i < len && is_digit(s[i]); ++i) {
        const int d = s[i] - '0';
        any = true;
        if (nd == 0 && d == 0) continue;               // a leading zero
        if (nd < MAX_DIGITS) { w = w * 10 + (uint64_t)d; ++nd; }
        else { ++e10; dropped = dropped || d != 0; }
    }
    if (i < len && s[i] == '.') {
        ++i;
        for (; i < len && is_digit(s[i]); ++i) {
            const int d = s[i] - '0';
            any = true;
            if (nd == 0 && d == 0) { --e10; continue; }
            if (nd < MAX_DIGITS) { w = w * 10 + (uint64_t)d; ++nd; --e10; }
            else dropped = dropped || d != 0;
        }
    }
    if (!any) return false;
    if (i < len && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < len && (s[i] == '+' || s[i] == '-')) { eneg = s[i] == '-'; ++i; }
        if (!(i < len && is_digit(s[i]))) return false;
        int64_t x = 0;
        for (; i < len && is_digit(s[i]); ++i)
            if (x < 1000000) x = x * 10 + (s[i] - '0'); // saturates far outside the table either way
        e10 += eneg ? -x : x;
    }
    flagged = false;
    if (w == 0) { bits = sign; return true; } // a zero, whatever its exponent
    if (dropped || e10 < -MAX_E10 || e10 > MAX_E10) {
        flagged = true;
        if (e10 < -MAX_E10 - 20) { bits = sign; return true; }               // below 10^19 * 10^-82: zero
        if (e10 > MAX_E10) { bits = sign | 0x7F800000u; return true; }       // at least 10^63: infinity
        if (e10 < -MAX_E10) { // drop low digits until the exponent fits the table
            while (e10 < -MAX_E10) { w /= 10; ++e10; }
            if (w == 0) { bits = sign; return true; }
        }
    }
    bits = sign | decimal_to_f32_bits(w, (int)e10, dropped || flagged);
    return true;
}

// [+-]? digits with |v| < 2^24, ending at a blank or the line's end
V2E_TF_HD bool parse_coord(const char *s, int64_t &i, int64_t len, float &out)
{
    bool neg = false;
    if (i < len && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; ++i; }
    if (!(i < len && is_digit(s[i]))) return false;
    uint32_t v = 0;
    for (; i < len && is_digit(s[i]); ++i)
        if (v < (1u << 24)) v = v * 10 + (uint32_t)(s[i] - '0'); // stays below 2^28 and at or above 2^24 once there
    if (v >= (1u << 24)) return false;
    if (i < len && !is_blank(s[i])) return false;
    out = neg ? -(float)v : (float)v;
    if (neg && v == 0) out = 0.0f; // int('-0') is 0
    return true;
}

// a field that is the single character 0 or 1
V2E_TF_HD bool parse_bit(const char *s, int64_t &i, int64_t len, int &out)
{
    if (!(i < len && (s[i] == '0' || s[i] == '1'))) return false;
    out = s[i] - '0';
    ++i;
    return i == len || is_blank(s[i]);
}

V2E_TF_HD bool skip_blanks(const char *s, int64_t &i, int64_t len) // true: at least one blank was there
{
    const int64_t i0 = i;
    while (i < len && is_blank(s[i])) ++i;
    return i > i0;
}

// one line s[0 .. len) without its '\n': LINE_*; row is set for LINE_ROW and LINE_ROW_FLAGGED
V2E_TF_HD int parse_line(const char *s, int64_t len, int want_labels, Row &row)
{
    if (len > 0 && s[len - 1] == '\r') --len;
    int64_t i = 0;
    skip_blanks(s, i, len);
    if (i == len || s[i] == '#') return LINE_SKIP;
    uint32_t tb;
    bool flagged;
    if (!parse_time(s, i, len, tb, flagged)) return LINE_BAD;
    __builtin_memcpy(&row.t, &tb, 4);
    if (!skip_blanks(s, i, len) || !parse_coord(s, i, len, row.x)) return LINE_BAD;
    if (!skip_blanks(s, i, len) || !parse_coord(s, i, len, row.y)) return LINE_BAD;
    int p;
    if (!skip_blanks(s, i, len) || !parse_bit(s, i, len, p)) return LINE_BAD;
    row.p = p ? 1.0f : -1.0f;
    row.label = -1;
    skip_blanks(s, i, len);
    if (i < len) {
        if (!parse_bit(s, i, len, row.label)) return LINE_BAD;
        skip_blanks(s, i, len);
        if (i < len) return LINE_BAD; // a sixth field, or junk
    }
    if (want_labels && row.label < 0) return LINE_BAD;
    return flagged ? LINE_ROW_FLAGGED : LINE_ROW;
}

} // namespace v2e_tp
