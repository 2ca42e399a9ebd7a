// lnerf_wave_addr.h -- addresses of the weight LDS-DMA and of the slab stores as a wave-uniform
// base (scalar registers) plus a per-lane constant (one vector register for the kernel's lifetime).
//
// k1 (lnerf_k16.hip) and kr (lnerf_render.hip) issue every LDS-DMA piece and every slab store at
// an address of that shape. Written as pointer + per-lane index the compiler rebuilt a 64-bit
// per-lane address for each instruction (a 64-bit vector add per DMA piece and per store, and a
// null test of the generic -> LDS pointer cast per piece); here the split is explicit: the
// arithmetic below is plain integer code that the host can run (tests/test_wave_addr.py checks it
// against the pointer expressions for every lane), the device part hands the two halves to the
// SGPR-base forms of the instructions.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LNERF_HD __host__ __device__ constexpr
#else
#define LNERF_HD constexpr
#endif

namespace lnerf {
namespace waddr {

// ---- LDS-DMA pieces: a chunk of `bytes` (a multiple of 1 KiB) is copied by the workgroup's NW
// waves in wave instructions of 1 KiB (64 lanes x 16 B, lane-linear at both ends). Piece p of wave
// w is the KiB at chunk byte w KiB + p NW KiB, the same offset in the source and in the ring slot.
constexpr unsigned kPieceBytes = 1024;

// the per-lane part of every DMA source address (and of every weight fragment read)
LNERF_HD unsigned dma_lane_off(int lane) { return (unsigned)lane * 16u; }
// wave w's first piece, from the chunk's start
LNERF_HD unsigned dma_wave_off(int wave) { return (unsigned)wave * kPieceBytes; }
// piece p of a wave, from the wave's first piece
LNERF_HD unsigned dma_piece_stride(int nw) { return (unsigned)nw * kPieceBytes; }
LNERF_HD unsigned dma_piece_off(int p, int nw) { return (unsigned)p * dma_piece_stride(nw); }
// the pieces wave w issues for a chunk of `bytes`
LNERF_HD int dma_piece_count(int bytes, int wave, int nw) {
    const int woff = (int)dma_wave_off(wave), st = (int)dma_piece_stride(nw);
    return woff < bytes ? (bytes - woff + st - 1) / st : 0;
}

// ---- slab stores: k-step s of a wave's half-block run writes two wave instructions, the feature
// halves h = 0, 1 of the 32-feature tile, lane (n = lane & 15, g = lane >> 4) its sample n's
// features 4g ..+3 of the half.
// f32 slabs (G, and A under bf16x6): [s][h][16 samples][16 features] x 4 B, 16 B per lane.
LNERF_HD unsigned slab_lane_off_f32(int lane) { return (unsigned)((lane & 15) * 16 + 4 * (lane >> 4)) * 4u; }
LNERF_HD unsigned slab_step_off_f32(int s) { return (unsigned)s * 4096u; }
constexpr unsigned kSlabHalfF32 = 1024;   // h = 1, from h = 0
// int24 A slabs: [s][h][16 samples][16 features] x 3 B, 12 B per lane.
LNERF_HD unsigned slab_lane_off_24(int lane) { return (unsigned)((lane & 15) * 48 + 12 * (lane >> 4)); }
LNERF_HD unsigned slab_step_off_24(int s) { return (unsigned)s * 3072u; }
constexpr unsigned kSlabHalf24 = 768;

}   // namespace waddr

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// The wave-uniform state and the per-lane constants of a k1 / kr wave, computed once per kernel.
struct WaveCtx {
    int wave;            // wave of the workgroup (scalar)
    unsigned woff;       // waddr::dma_wave_off(wave)
    unsigned ring;       // LDS byte address of the weight ring
    unsigned bias_ring;  // LDS byte address of the bias ring
    unsigned lane16;     // waddr::dma_lane_off(lane)
    unsigned lane_f32;   // waddr::slab_lane_off_f32(lane)
    unsigned lane_24;    // waddr::slab_lane_off_24(lane)
};

// LDS byte address of a pointer into __shared__ memory (kernel prologue only: the cast tests the
// generic pointer for null, two scalar instructions the chunk loop has no use for)
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) void*)p;
}

__device__ __forceinline__ WaveCtx make_wave_ctx(const void* ring, const void* bias_ring) {
    const int lane = threadIdx.x & 63;
    WaveCtx c;
    c.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    c.woff = waddr::dma_wave_off(c.wave);
    c.ring = __builtin_amdgcn_readfirstlane(lds_addr(ring));
    c.bias_ring = __builtin_amdgcn_readfirstlane(lds_addr(bias_ring));
    c.lane16 = waddr::dma_lane_off(lane);
    c.lane_f32 = waddr::slab_lane_off_f32(lane);
    c.lane_24 = waddr::slab_lane_off_24(lane);
    return c;
}

// One LDS-DMA wave instruction (global_load_lds_dwordx4: 16 B per lane from sbase + voff,
// lane-linear into the wave-uniform LDS byte address), from inline asm with M0 written in the same
// statement. sbase is a scalar register pair, voff the lane's 32-bit byte offset (lane16 everywhere).
// Why asm: an LDS-DMA the compiler can see makes it wait vmcnt(0) before every later LDS read
// (it cannot tell the ring slots apart), which would drain the next chunk's DMA; hidden from it,
// the transfer has no register destination (nothing the compiler could copy or reuse early) and
// its completion is counted by hand (the chunk barrier's vmcnt). The `s_nop 0` is the M0-write ->
// LDS-DMA wait state; the scalar base and the LDS address come out of scalar ALU instructions
// (never straight out of a v_readfirstlane, which a vector-memory instruction may read only 5 wait
// states later: tests/test_k16_addressing.py checks both in the disassembly). No compiler code in
// these kernels reads M0 (tests/test_isa.py). The instruction offset stays 0: it would move the LDS
// end of the transfer as well.
// (This form serves the pieces outside the steady state -- a chunk issued whole, the bias piece, the
// render's resident head -- where the compiler keeps a loop-carried LDS address in a vector
// register: the readfirstlane makes it a scalar operand; M0's writer is a scalar move either way.)
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, unsigned lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase),
                 "s"(__builtin_amdgcn_readfirstlane(lds)));
}
// the same with the LDS address as a scalar base plus a compile-time offset (one scalar add into M0)
template <unsigned OFF>
__device__ __forceinline__ void glds16s_at(const void* sbase, unsigned voff, unsigned lds_base) {
    asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase),
                 "s"(lds_base), "n"(OFF)
                 : "scc");
}
#endif

}   // namespace lnerf
