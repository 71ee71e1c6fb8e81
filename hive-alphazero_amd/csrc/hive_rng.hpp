// hive_rng.hpp -- the counter-based generator shared by the search (root noise, move resampling: hive_search.hip) and
// the arena (opening draws: hive_arena.hip).  A stream is a pure function of its four keys, so whatever is drawn from it
// does not depend on the batch slot, process or GPU that asks.
#pragma once
#include <hip/hip_runtime.h>

namespace hive {

__device__ __forceinline__ unsigned long long splitmix(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
struct Rng {
    unsigned long long s;
    __device__ Rng(unsigned long long seed, unsigned long long a, unsigned long long b, unsigned long long c)
    {
        s = splitmix(seed ^ splitmix(a * 0x100000001B3ull + splitmix(b * 0x9E3779B1ull + c)));
    }
    __device__ float uniform()     // (0, 1)
    {
        s = splitmix(s);
        return ((float)(s >> 40) + 0.5f) * (1.0f / 16777216.0f);
    }
    __device__ float normal()
    {
        float u1 = uniform(), u2 = uniform();
        return sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530718f * u2);
    }
    // Marsaglia-Tsang, alpha < 1 through the alpha+1 boost
    __device__ float gamma(float alpha)
    {
        float a = alpha + 1.0f, d = a - 1.0f / 3.0f, c = rsqrtf(9.0f * d), out = d;
        for (int it = 0; it < 8; ++it) {
            float x = normal(), v = 1.0f + c * x;
            if (v <= 0.0f) continue;
            v = v * v * v;
            float u = uniform();
            if (__logf(u) < 0.5f * x * x + d - d * v + d * __logf(v)) { out = d * v; break; }
        }
        return out * __powf(uniform(), 1.0f / alpha);
    }
};

}  // namespace hive
