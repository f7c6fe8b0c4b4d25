// LDS-DMA ring toolkit of the convolution and weight-gradient kernels (hipcc only; included by conv.hip and wgrad.hip after common.h).
// Pieces, not a ring object: every kernel keeps its own loop and its ping-pong schedule; what lives here is what those loops used to copy
// from each other -- the buffer resource and its out-of-range marker, the lane geometry of an "8 rows of 128 B" LDS-DMA request, the counted
// wait with the bare barrier, the ring-position advance, the zeroing of the f16x3 accumulator pairs and the fold of a hi / cross pair.  Every
// use leaves its kernel's machine code byte for byte as it was; where a helper did not (profiles/r25/conv_ring_toolkit.md) the site is hand-written.
#pragma once

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float LO_SCALE = 2048.0f;      // AMP_CONV_F16X3: lo' = (x - hi) * 2^11 (see conv_f16x3_kernel)

// ---- buffer addressing --------------------------------------------------------------------------------------------
// A voffset of OOB_VOFF is >= num_records of every buffer these kernels accept (< 2 GiB): the hardware bounds check writes zeros into LDS
// for it -- out-of-image taps and rows beyond the tensor need no predication and no zero page.
constexpr unsigned int OOB_VOFF = 0x80000000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const float* p, unsigned int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, bytes, 0x00020000);
}

// ---- staging geometry: one wave-instruction writes 8 LDS rows x 128 B linearly; lane = (row lane >> 3 of the 8, 16-B position lane & 7) ----
__device__ __forceinline__ int dma_row(int lane) { return lane >> 3; }
__device__ __forceinline__ int dma_pos(int lane) { return lane & 7; }
// the source chunk (floats) a lane at position `pos` fetches for LDS row r: XOR-swizzled, undone by the fragment reads (conv_glds_kernel)
__device__ __forceinline__ int dma_chunk(int pos, int r) { return 4 * (pos ^ ((r >> 1) & 7)); }

// ---- the ring step ------------------------------------------------------------------------------------------------
// Bare s_barrier: __syncthreads() is fence + barrier, and the workgroup-release fence waits for vmcnt(0) -- it would drain the very
// requests a ring keeps in flight.  Nothing a fence orders is needed here: the tiles are written by LDS-DMA (covered by the counted vmcnt
// in front of the barrier) and read by ds_read whose data has returned (lgkmcnt(0) in the same wait).  The empty asm statements keep the
// compiler from moving LDS accesses across the barrier.
__device__ __forceinline__ void ring_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();          // every wave's share of the tile is in LDS; everyone is done with the tile before it
    asm volatile("" ::: "memory");
}

// Opens a K-step.  The tile has landed once all but the youngest tile's NDMA requests of this wave are done (LDS-DMA counts in vmcnt, in
// order; `more`: a younger tile is in flight); lgkmcnt(0): this wave's fragment reads of the previous tile have returned.
template <int NDMA>
__device__ __forceinline__ void ring_open(bool more) {
    static_assert(NDMA < 16, "vmcnt immediate");
    if (more) __builtin_amdgcn_s_waitcnt(0x0070 | NDMA);
    else __builtin_amdgcn_s_waitcnt(0x0070);
    ring_barrier();
}

// ring positions of the tile being computed / staged, NSTAGE buffers
template <int NSTAGE>
__device__ __forceinline__ void ring_next(int& cur, int& nxt) {
    cur = (cur == NSTAGE - 1) ? 0 : cur + 1;
    nxt = (nxt == NSTAGE - 1) ? 0 : nxt + 1;
}

// ---- f16x3 accumulator pairs: acc = hi*hi sums, acx = cross-term sums (scaled by LO_SCALE) ----
template <int MB, int NB>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[MB][NB], f32x4 (&acx)[MB][NB]) {
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[i][j][e] = 0.f; acx[i][j][e] = 0.f; }
}

__device__ __forceinline__ float fold(float hi, float cross) { return __fadd_rn(hi, __fmul_rn(cross, 1.0f / LO_SCALE)); }

}  // namespace
