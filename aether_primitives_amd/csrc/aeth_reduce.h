// aeth_reduce.h -- the record reductions' shared core (not installed): aeth_vec_stats (aeth_stats.hip), aeth_sync_line /
// aeth_sync_lag (aeth_sync.hip) and aeth_mov_search (aeth_mov.hip) turn 256 records of a workgroup into one, and many
// records into one, through the code below and through nothing else.  A user brings a record (a multiple of 8 bytes), an
// identity, a combine and the order in which a LANE takes the terms of its chunk; everything behind the lane is here.
//
// THE TREE.  `combine(a, b)` must give the same bits as `combine(b, a)`.
//   butterfly   the 64 lanes of a wave combine by the xor butterfly 32, 16, 8, 4, 2, 1: a = combine(a, a of lane ^ mask);
//               every lane of the wave then holds the same value
//   wave step   the four waves as combine(combine(w0, w1), combine(w2, w3)), in thread 0
//   fold        workgroup b takes the records [b * per, min((b + 1) * per, total)): lane t combines records t, t + 256,
//               ... of them in that order, starting from the identity, then the butterfly and the wave step
// So one record per chunk is the tree over the lanes' own results; one record per block is the fold of its chunk records
// (per = chunks of a full block); the total is the fold of the block records in one workgroup (per == total).  The order
// is a function of the index inside the block and of the block's length only: neither the CU count nor a pointer enters.
//
// THE CUT.  A call of n items in blocks of `block` (0: one block) is cut block by block into chunks of the family's
// chunk size, the last chunk of a block short; one workgroup per chunk (Cut / cut_of on the host, Geo / geo_of in the
// chunk kernel).
//
// THE HOST SIDE (run_blocks) is one sequence for every family: the chunk kernel writes chunk records into the family's
// slab, or the block records themselves when a block is one chunk (`direct`); the per-block fold; the fold of the total
// into HostIO's pinned bounce buffer; one wait when a total was asked for.
//
// Not on this core: aeth_corr_search's folds (aeth_fir.hip, best_block_reduce) and the Viterbi decoder's sub-wave argmax
// (aeth_cc.hip).
#pragma once

#include "aeth_internal.h"

namespace aeth {
namespace red {

constexpr int kBlock = 256;                                          // lanes of every workgroup here: four waves

// ---- device: the tree ----------------------------------------------------------------------------------------------
// the record of lane (lane ^ mask), 8 bytes at a time
template <class R> __device__ __forceinline__ R shfl_xor(const R &a, int mask)
{
    static_assert(sizeof(R) % 8 == 0, "a record is a whole number of 8-byte words");
    struct Words { unsigned long long w[sizeof(R) / 8]; };
    Words v = __builtin_bit_cast(Words, a);
#pragma unroll
    for (unsigned i = 0; i < sizeof(R) / 8; i++) v.w[i] = __shfl_xor(v.w[i], mask);
    return __builtin_bit_cast(R, v);
}

// the workgroup's 256 records -> one, valid in thread 0; `lds` holds four records
template <class R, class C> __device__ __forceinline__ R block_reduce(R a, R *lds, C combine)
{
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) a = combine(a, shfl_xor(a, mask));
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) a = combine(combine(lds[0], lds[1]), combine(lds[2], lds[3]));
    return a;
}

// workgroup b folds in[b * per .. min((b + 1) * per, total)); valid in thread 0
template <class R, class C>
__device__ __forceinline__ R fold(const R *__restrict__ in, size_t per, size_t total, R identity, R *lds, C combine)
{
    const size_t first = (size_t)blockIdx.x * per;
    const size_t cnt = total - first < per ? total - first : per;
    R a = identity;
    for (size_t r = threadIdx.x; r < cnt; r += kBlock) a = combine(a, in[first + r]);
    return block_reduce(a, lds, combine);
}

// ---- the cut -------------------------------------------------------------------------------------------------------
// where a workgroup works: block b, chunk k of it -> first item of the call (g), items (left)
struct Geo { unsigned b; size_t g; unsigned left; };
template <unsigned CHUNK> __device__ __forceinline__ Geo geo_of(size_t n, size_t block, const FastDiv &cpb)
{
    Geo o;
    o.b = fdiv(blockIdx.x, cpb);
    const unsigned k = blockIdx.x - o.b * cpb.d;
    const size_t bstart = (size_t)o.b * block;
    const size_t blen = n - bstart < block ? n - bstart : block;
    const size_t cstart = (size_t)k * CHUNK;                         // < blen: the grid holds ceil(blen / CHUNK) chunks of the block
    o.g = bstart + cstart;
    o.left = blen - cstart < CHUNK ? (unsigned)(blen - cstart) : CHUNK;
    return o;
}

// how a call is cut: nb blocks of `block` items (the last one short), cpb chunks in a full block, nwg workgroups
struct Cut { size_t block, nb, cpb, nwg; };
inline bool cut_of(size_t n, size_t block, size_t chunk, Cut &c)
{
    c.block = block ? block : n;
    c.nb = (n + c.block - 1) / c.block;
    c.cpb = (c.block + chunk - 1) / chunk;
    if (c.nb >= ((size_t)1 << 31) || c.cpb >= ((size_t)1 << 31)) return false;
    const size_t last = n - (c.nb - 1) * c.block;
    c.nwg = (c.nb - 1) * c.cpb + (last + chunk - 1) / chunk;
    return c.nwg < ((size_t)1 << 31);
}

// ---- host: behind the chunk kernel, the per-block fold and the total ------------------------------------------------
// `slab`: the family's scratch buffer, laid out [chunk records][block records, unless the caller holds them (rec_dev)];
// `launch(stream, out, direct)` enqueues the chunk kernel, `fold(stream, workgroups, in, per, total, out)` the family's
// fold kernel; total_host (or null) receives the record over the whole call, and the call then waits.
template <class R, class L, class F>
int run_blocks(aeth_ctx *ctx, DevScratch &slab, const Cut &c, R *rec_dev, void *total_host, F fold, L launch)
{
    DeviceGuard dev_guard(ctx->device);
    const bool direct = c.cpb == 1;                                  // a block is one chunk: its record needs no fold
    const size_t nchunk = direct ? 0 : c.nwg;
    int rc = scratch_ensure(ctx, slab, (nchunk + (rec_dev ? 0 : c.nb)) * sizeof(R)); if (rc) return rc;
    R *chunks = static_cast<R *>(slab.p);
    R *blocks = rec_dev ? rec_dev : chunks + nchunk;
    HostIO io;
    if (total_host) { rc = io.open(ctx, 0, sizeof(R)); if (rc) return rc; }    // the pinned bounce buffer
    hipStream_t s = ctx_stream(ctx);
    launch(s, direct ? blocks : chunks, direct ? 1 : 0);
    if (!direct) fold(s, (unsigned)c.nb, (const R *)chunks, c.cpb, c.nwg, blocks);
    if (total_host) fold(s, 1u, (const R *)blocks, c.nb, c.nb, static_cast<R *>(io.buf[1]));
    AETH_HIP(hipGetLastError());
    if (total_host) return io.get(total_host, 1, sizeof(R));
    return AETH_OK;
}

}  // namespace red
}  // namespace aeth
