// text_format.h -- the text event line of ae_text_output.py:86-101, for host and device.
//
//   t = (events[:, 0]).astype(float)                       -> '{}'.format(t[i]): the shortest round-trip repr of the float64
//   x = events[:, 1].astype(np.int32), y likewise          -> int32 truncation
//   p = ((events[:, 3] + 1) / 2).astype(np.int32)
//   line '{} {} {} {}\n', or '{} {} {} {} {}\n' with int(signnoise_label[i]) when labelling is on
//
// The time stamp is a float32 widened to float64, so its significand has 24 bits while the rounding interval that a decimal
// string must hit is float64's.  Python's repr (David Gay's dtoa, mode 0) prints the decimal with the fewest significant
// digits that reads back as that float64; among those of that length, the one closest to the value (a tie goes to the even
// last digit).  Here this is computed with exact integer arithmetic: the value and both ends of its rounding interval are
// scaled by 10^-q into 18-19 digit integers (q = floor(log10 v) - 17, an exact power-of-5 multiply and a shift, or for
// v >= 1e18 a division by 5^q), after which the shortest decimal is found on 64-bit integers.  Nothing depends on the range
// of the time stamps: every finite float32 (subnormals included) takes the same route.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define V2E_TF_HD __host__ __device__ __forceinline__
#else
#define V2E_TF_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define V2E_TF_TABLE static __constant__ const
#else
#define V2E_TF_TABLE static const
#endif

#include "pow5_table.h"

// longest line: t 24 ("-1.2345678901234567e-45"), three int32 of 11 and 1 label, 4 spaces, '\n'
#define V2E_TEXT_MAX_LINE 64

namespace v2e_tf {

V2E_TF_HD uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

struct Scaled {
    uint64_t n;   // floor(X * 2^g / 10^q)
    int frac;     // the fraction left over: 0 zero, 1 below one half, 2 exactly one half, 3 above
};

// X * 2^g / 10^q for X < 2^56, with q = k - 17 and g = e2 - 54 as v2e_tf_shortest sets them up
V2E_TF_HD Scaled scale(uint64_t X, int g, int q)
{
    Scaled r;
    if (q <= 0) { // X * 5^p * 2^(g + p), p = -q <= 62: a product of at most 56 + 144 bits, then a shift
        const int p = -q, s = g + p;
        const unsigned long long *f = V2E_POW5[p];
        uint64_t P[4];
        uint64_t lo0 = X * f[0], hi0 = mulhi64(X, f[0]);
        uint64_t lo1 = X * f[1], hi1 = mulhi64(X, f[1]);
        uint64_t lo2 = X * f[2], hi2 = mulhi64(X, f[2]);
        P[0] = lo0;
        P[1] = hi0 + lo1;
        uint64_t c = P[1] < lo1;
        P[2] = hi1 + lo2;
        uint64_t c2 = P[2] < lo2;
        P[2] += c;
        c2 += P[2] < c;
        P[3] = hi2 + c2;
        if (s >= 0) { // an integer (then P < 2^64 and s small: the result is below 10^19)
            r.n = P[0] << s;
            r.frac = 0;
            return r;
        }
        const int sh = -s, li = sh >> 6, b = sh & 63; // result = bits [sh, sh + 64) of P; sh <= 141
        r.n = b ? ((P[li] >> b) | (P[li + 1] << (64 - b))) : P[li];
        const int hb = sh - 1; // the half bit
        const uint64_t half = (P[hb >> 6] >> (hb & 63)) & 1u;
        uint64_t below = P[hb >> 6] & ((1ull << (hb & 63)) - 1ull);
        for (int k = 0; k < (hb >> 6); ++k) below |= P[k];
        r.frac = half ? (below ? 3 : 2) : (below ? 1 : 0);
        return r;
    }
    // q > 0 (v >= 1e18): (X << (g - q)) / 5^q with 5 <= g - q <= 52, so the numerator has fewer than 108 bits; q <= 21 and
    // 5^q is divided out as 5^13 (< 2^32) and 5^(q - 13), long division on 32-bit limbs
    const int sh = g - q;
    uint32_t w[4];
    {
        const uint64_t lo = X << sh, hi = sh ? (X >> (64 - sh)) : 0;
        w[0] = (uint32_t)lo; w[1] = (uint32_t)(lo >> 32); w[2] = (uint32_t)hi; w[3] = (uint32_t)(hi >> 32);
    }
    uint64_t rem = 0, mult = 1;
    int left = q;
    while (left > 0) {
        const int step = left > 13 ? 13 : left;
        const uint32_t d = (uint32_t)V2E_POW5[step][0];
        uint64_t rr = 0;
        for (int k = 3; k >= 0; --k) {
            const uint64_t cur = (rr << 32) | w[k];
            w[k] = (uint32_t)(cur / d);
            rr = cur % d;
        }
        rem += rr * mult; // x = ((x1 * d2 + r2) * d1 + r1): remainder r2 * d1 + r1 of x / (d1 d2)
        mult *= d;
        left -= step;
    }
    r.n = ((uint64_t)w[1] << 32) | w[0];
    r.frac = rem == 0 ? 0 : (2 * rem < mult ? 1 : (2 * rem == mult ? 2 : 3));
    return r;
}

struct Decimal {
    uint64_t digits; // no trailing zeros
    int exp10;       // value = digits * 10^exp10
};

// the shortest round-trip decimal of (double)f for a finite, nonzero float32 magnitude `a` (its bits, sign cleared)
V2E_TF_HD Decimal shortest(uint32_t a)
{
    uint32_t m = a & 0x7FFFFFu;
    int e;
    if ((a >> 23) == 0) { // subnormal float32: a normal float64; normalise m to 24 bits
        e = -149;
        while (!(m & 0x800000u)) { m <<= 1; --e; }
    } else {
        m |= 0x800000u;
        e = (int)(a >> 23) - 150;
    }
    // value = m 2^e, m in [2^23, 2^24): as float64 m 2^29 units of 2^(e - 29).  In units of 2^(e - 31) the value is V = m 2^31
    // and the rounding interval [V - lo, V + 2] (float64 half units; lo = 1 below a power of two, where the next float64 down is
    // half as far).  Its ends round to the even float64 (m 2^29 is even), so both are included.
    const uint64_t V = (uint64_t)m << 31;
    const uint64_t lo = (m == 0x800000u) ? 1 : 2;
    const int e2 = e + 23; // floor(log2 value)
    const int g = e - 31;
    // k = floor(log10 2^e2) <= floor(log10 value) <= k + 1 (78913 / 2^18 is log10 2 to enough digits for |e2| < 1650)
    const int k = e2 >= 0 ? (int)(((uint32_t)e2 * 78913u) >> 18) : -(int)(((uint32_t)(-e2) * 78913u) >> 18) - 1;
    const int q = k - 17; // value / 10^q in [10^17, 10^19); the interval is more than 8 of those units wide
    const Scaled sv = scale(V, g, q);
    const Scaled sl = scale(V - lo, g, q);
    const Scaled sh = scale(V + 2, g, q);
    uint64_t L = sl.n + (sl.frac ? 1u : 0u); // smallest integer >= the lower end
    uint64_t H = sh.n;                        // largest integer <= the upper end
    // the largest 10^j with a multiple in [L, H]: strip digits while floor(H / 10) > floor((L - 1) / 10)
    uint64_t h = H, l = L - 1, v = sv.n;
    int frac = sv.frac, j = 0;
    while (h / 10 > l / 10) {
        const int d = (int)(v % 10);
        frac = d < 5 ? ((d == 0 && frac == 0) ? 0 : 1) : (d > 5 ? 3 : (frac == 0 ? 2 : 3));
        h /= 10; l /= 10; v /= 10; ++j;
    }
    // candidates v and v + 1 (in units of 10^(q + j)); at least one lies in (l, h]
    const bool lo_in = v > l, hi_in = v + 1 <= h;
    bool up;
    if (lo_in && hi_in) up = frac == 3 || (frac == 2 && (v & 1));
    else up = !lo_in;
    Decimal r;
    r.digits = up ? v + 1 : v;
    r.exp10 = q + j;
    while (r.digits % 10 == 0) { r.digits /= 10; ++r.exp10; }
    return r;
}

V2E_TF_HD int ndigits(uint64_t v)
{
    int n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}

// digits of v (n of them) at o[0 ..], a '.' after the first `point` digits (point <= 0 or >= n: none)
template <bool WRITE>
V2E_TF_HD int put_digits(char *o, uint64_t v, int n, int point)
{
    const int len = n + ((point > 0 && point < n) ? 1 : 0);
    if (WRITE) {
        for (int i = n - 1; i >= 0; --i) {
            o[i + ((point > 0 && i >= point) ? 1 : 0)] = (char)('0' + (int)(v % 10));
            v /= 10;
        }
        if (point > 0 && point < n) o[point] = '.';
    }
    return len;
}

// repr((float64)f) without a terminating NUL; returns the length (at most 24)
template <bool WRITE>
V2E_TF_HD int put_f32(char *o, float f)
{
    uint32_t bits;
    __builtin_memcpy(&bits, &f, 4);
    const uint32_t a = bits & 0x7FFFFFFFu;
    int n = 0;
    if (a > 0x7F800000u) { // numpy prints every NaN as 'nan'
        if (WRITE) { o[0] = 'n'; o[1] = 'a'; o[2] = 'n'; }
        return 3;
    }
    if (bits >> 31) { if (WRITE) o[0] = '-'; n = 1; }
    if (a == 0x7F800000u) {
        if (WRITE) { o[n] = 'i'; o[n + 1] = 'n'; o[n + 2] = 'f'; }
        return n + 3;
    }
    if (a == 0) {
        if (WRITE) { o[n] = '0'; o[n + 1] = '.'; o[n + 2] = '0'; }
        return n + 3;
    }
    const Decimal d = shortest(a);
    const int nd = ndigits(d.digits);
    const int decpt = d.exp10 + nd; // value = 0.d1 d2 ... x 10^decpt
    if (decpt > -4 && decpt <= 16) { // Python's float_repr_style 'short': fixed notation
        if (decpt <= 0) {
            if (WRITE) { o[n] = '0'; o[n + 1] = '.'; }
            n += 2;
            for (int i = 0; i < -decpt; ++i) { if (WRITE) o[n] = '0'; ++n; }
            n += put_digits<WRITE>(o + n, d.digits, nd, 0);
        } else if (decpt < nd) {
            n += put_digits<WRITE>(o + n, d.digits, nd, decpt);
        } else {
            n += put_digits<WRITE>(o + n, d.digits, nd, 0);
            for (int i = nd; i < decpt; ++i) { if (WRITE) o[n] = '0'; ++n; }
            if (WRITE) { o[n] = '.'; o[n + 1] = '0'; }
            n += 2;
        }
        return n;
    }
    n += put_digits<WRITE>(o + n, d.digits, nd, 1); // d1[.d2 ...]e<sign><at least two digits>
    int x = decpt - 1;
    if (WRITE) { o[n] = 'e'; o[n + 1] = x < 0 ? '-' : '+'; }
    n += 2;
    if (x < 0) x = -x;
    if (x >= 100) { if (WRITE) o[n] = (char)('0' + x / 100); ++n; x %= 100; }
    if (WRITE) { o[n] = (char)('0' + x / 10); o[n + 1] = (char)('0' + x % 10); }
    return n + 2;
}

template <bool WRITE>
V2E_TF_HD int put_i32(char *o, int32_t v)
{
    int n = 0;
    uint32_t u = (uint32_t)v;
    if (v < 0) { if (WRITE) o[0] = '-'; n = 1; u = 0u - u; }
    int nd = 1;
    for (uint32_t t = u; t >= 10; t /= 10) ++nd;
    if (WRITE)
        for (int i = nd - 1; i >= 0; --i) { o[n + i] = (char)('0' + u % 10); u /= 10; }
    return n + nd;
}

// one text line of the row (t, x, y, p); label < 0: no label column
template <bool WRITE>
V2E_TF_HD int put_line(char *o, float t, float x, float y, float p, int label)
{
    int n = put_f32<WRITE>(o, t);
    const int32_t cols[3] = {(int32_t)x, (int32_t)y, (int32_t)((p + 1.0f) / 2.0f)};
    for (int c = 0; c < 3; ++c) {
        if (WRITE) o[n] = ' ';
        ++n;
        n += put_i32<WRITE>(o + n, cols[c]);
    }
    if (label >= 0) {
        if (WRITE) { o[n] = ' '; o[n + 1] = (char)('0' + label); }
        n += 2;
    }
    if (WRITE) o[n] = '\n';
    return n + 1;
}

} // namespace v2e_tf
