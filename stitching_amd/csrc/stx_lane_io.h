// stx_lane_io.h — how a lane of the frame kernels (stx_ingest.hip, stx_emit.hip) moves its bytes: whole words where the host has marked
// the plane "wide" and the lane owns all of them, else exactly the bytes it owns, one at a time.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {
// NW words from p: as words (p is 4-aligned and all 4 NW bytes belong to the lane), else the first nbytes, byte by byte (rest 0)
template <int NW>
__device__ __forceinline__ void load_words(const uint8_t* __restrict__ p, int nbytes, bool words, uint32_t (&s)[NW])
{
    if (words) {
#pragma unroll
        for (int i = 0; i < NW; i++) s[i] = ((const uint32_t*)p)[i];
    } else {
#pragma unroll
        for (int i = 0; i < NW; i++) s[i] = 0u;
#pragma unroll
        for (int j = 0; j < NW * 4; j++)
            if (j < nbytes) s[j >> 2] |= (uint32_t)p[j] << ((j & 3) * 8);
    }
}

// two bytes at p (I420's chroma of four pixels): one 16-bit load where p is 2-aligned and both belong to the lane
__device__ __forceinline__ uint32_t load_pair(const uint8_t* __restrict__ p, int nbytes, bool halves)
{
    if (halves) return *(const uint16_t*)p;
    uint32_t v = p[0];
    if (nbytes > 1) v |= (uint32_t)p[1] << 8;
    return v;
}

template <int NW>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&s)[NW], int j) { return (s[j >> 2] >> ((j & 3) * 8)) & 255u; }

// NW words to d (4-aligned): all of them, or the first nbytes byte by byte
template <int NW>
__device__ __forceinline__ void store_words(uint8_t* __restrict__ d, const uint32_t (&o)[NW], int nbytes)
{
    if (nbytes == NW * 4) {
#pragma unroll
        for (int i = 0; i < NW; i++) ((uint32_t*)d)[i] = o[i];
    } else {
#pragma unroll
        for (int j = 0; j < NW * 4; j++)
            if (j < nbytes) d[j] = (uint8_t)byte_of(o, j);
    }
}

// the same with the choice made by the caller: the destination of emit is foreign memory of any base and pitch
template <int NW>
__device__ __forceinline__ void store_words(uint8_t* __restrict__ d, const uint32_t (&o)[NW], int nbytes, bool words)
{
    if (words) {
#pragma unroll
        for (int i = 0; i < NW; i++) ((uint32_t*)d)[i] = o[i];
    } else {
#pragma unroll
        for (int j = 0; j < NW * 4; j++)
            if (j < nbytes) d[j] = (uint8_t)byte_of(o, j);
    }
}

// up to two bytes of v to d (I420's chroma of four pixels): one 16-bit store where d is 2-aligned and both belong to the lane
__device__ __forceinline__ void store_pair(uint8_t* __restrict__ d, uint32_t v, int nbytes, bool halves)
{
    if (halves) { *(uint16_t*)d = (uint16_t)v; return; }
    d[0] = (uint8_t)v;
    if (nbytes > 1) d[1] = (uint8_t)(v >> 8);
}
}  // namespace
