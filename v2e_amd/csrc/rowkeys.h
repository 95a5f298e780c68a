// rowkeys.h -- which rows are valid and the sort key of a row, shared by denoise.hip and patches.hip
#pragma once
#include <hip/hip_runtime.h>

constexpr long long KEY_BAD = 0x7fffffffffffffffLL;         // sorts behind every valid key as a signed 64-bit value

// the pixel of a valid row, -1 for a bad one (the float comparisons come first: they refuse NaN and everything the int
// conversion cannot hold)
__device__ __forceinline__ long long row_pixel(const float4 e, int H, int W)
{
    const int x = (int)e.y, y = (int)e.z;
    if (!(e.y >= 0.0f && e.y < (float)W && e.z >= 0.0f && e.z < (float)H && (float)x == e.y && (float)y == e.z &&
          fabsf(e.x) <= 3.402823466e+38f))
        return -1;
    return (long long)y * W + x;
}
