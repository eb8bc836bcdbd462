// swt_fused.inc -- one level of the 2-D stationary transform (forward) in ONE launch, float32.
//
// The per-level form (swt.hip + cols_ring.inc) runs a row pass that writes two full-size temporaries and a column
// pass that reads them back: 3 + 6 image-sized transfers per level where 1 read + 4 writes are needed.  Here the row
// pass result never leaves the chip:
//   * rows y = rho (mod f), f = 2^(level-1), form f independent sub-images on which the dilated column filter is an
//     ordinary dense one (f divides Nr, so the periodic wrap stays inside the class);
//   * a workgroup owns a 1024-column tile x one residue class x a chunk of that class's rows and walks DOWN it: each
//     input row is staged once in LDS with its (hlen-1)*f halo (16-byte coalesced loads, prefetched one row ahead in
//     registers, two LDS buffers -> one barrier per row), every thread runs the dilated ROW pass for its 4 columns out of
//     LDS (aligned 16-byte reads at stride f) and pushes (lo,hi) into a register ring of hlen rows;
//   * as soon as the ring holds a full window the COLUMN pass emits one row of A,H,V,D (16-byte stores).
// HBM traffic per level: N (+ halo) read, 4N written -- the algorithmic minimum of a level.
// Arithmetic per sample = row pass then column pass, taps ascending, one FMA per tap: bit-identical to the two-pass
// kernels and to the oracle.  Reference code replaced: w_kern_forward_swt_pass1/2 + one iteration of
// w_forward_swt_separable (src/separable.cu:409-516).
#include "swt_fused.hpp"

#include "stream_dev.hpp"

namespace pdwt {

constexpr int kSwtTile = 1024;  // columns per workgroup: 256 threads x 4


// (inverse kernels) workgroup row `by` -> (residue class rho, chunk ch of the class).  alt == 0: classes fastest (the order of rounds 1-2).
// alt == 1: the chunks of a class are consecutive in the tile order, and every second chunk walks UP its rows: two vertical neighbours
// then touch the HLEN-1 rows they both need at the same time (both at their start, or both at their end) on the same XCD, so the second
// read comes out of that XCD's L2 instead of memory.  An upward chunk pushes rows bottom-first, so the j-th oldest ring row pairs with
// tap j instead of tap HLEN-1-j (same products per output; the column sum runs bottom-up instead of top-down: the inverse SWT was
// never bit-identical to the two-pass form, tests compare at 1e-5 relative).
#define SWTF_INV_CHUNK(FCT)                                              \
    const int nch = (int)gridDim.y / (FCT);                              \
    const int rho = alt ? by / nch : by % (FCT);                         \
    const int ch = alt ? by % nch : by / (FCT);                          \
    const int m0 = ch * M;                                               \
    const int Mc = Nr / (FCT);                                           \
    const int nout = min(M, Mc - m0);                                    \
    if (nout <= 0) return;                                               \
    const bool up = alt && (ch & 1);
#define SWTF_INV_WALK(FCT)                                               \
    const int rb0 = up ? m0 + nout - 1 + (HLEN - 1 - C) : m0 - C;        \
    const int ob0 = up ? m0 + nout - 1 + (HLEN - 1) : m0 - (HLEN - 1);   \
    const int rst = up ? -1 : 1;                                         \
    v2f cpa[HLEN / 2], cpb[HLEN / 2]; /* column taps, oldest ring row first, as aligned SGPR pairs (pk_fma_sbcast) */ \
    _Pragma("unroll") for (int i = 0; i < HLEN / 2; i++) {               \
        cpa[i] = up ? v2f{f.a[2 * i], f.a[2 * i + 1]} : v2f{f.a[HLEN - 1 - 2 * i], f.a[HLEN - 2 - 2 * i]}; \
        cpb[i] = up ? v2f{f.b[2 * i], f.b[2 * i + 1]} : v2f{f.b[HLEN - 1 - 2 * i], f.b[HLEN - 2 - 2 * i]}; \
    }                                                                    \
    auto row_of = [&](int r) { return (size_t)SWTF_LD_ROW(rho + (FCT) * wrapi(rb0 + rst * min(r, nin - 1), Mc)) * Nc; };

// diagnostic builds only (tools/swt_diag.sh): PDWT_SWTF_DIAG & 1 folds every store, & 2 every load onto 64 image rows (cache-resident)
#ifndef PDWT_SWTF_DIAG
#define PDWT_SWTF_DIAG 0
#endif
#define SWTF_ST_ROW(row) ((PDWT_SWTF_DIAG & 1) ? ((row) & 63) : (row))
#define SWTF_LD_ROW(row) ((PDWT_SWTF_DIAG & 2) ? ((row) & 63) : (row))
#ifdef PDWT_SWTF_WAIT0
#define SWTF_COUNTED false
#else
#define SWTF_COUNTED true
#endif
__device__ __forceinline__ void swtf_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#ifndef PDWT_SWTF_WP  // inverse level kernels, tap spacing 1 and 2: wave-private staging, no workgroup barrier (round 6: C3 levels 1-2 162 -> 155 us; 0 = the shared rows of rounds 2-5)
#define PDWT_SWTF_WP 1
#endif
#define SWTF_WAVE_PRIVATE (PDWT_SWTF_WP != 0)

// Translation units (the unrolled bodies are expensive to compile: one part per file, built in parallel):
//   1 forward, banks of 2..16 taps      2 inverse (one 16-byte read per tap), 2..16 taps      3 inverse, residue-major rows, 8..16 taps
//   4 forward, 18 and 20 taps           5 inverse, 18 and 20 taps
#if PDWT_SWTF_PART == 1 || PDWT_SWTF_PART == 4
// FSEL: 1, 2 = tap spacing 1 or 2 (the row-pass window is read as one run of aligned 16-byte chunks),
//       0 = spacing >= 4 (a multiple of 4: every tap is its own aligned 16-byte read)
template <int HLEN, int FSEL>
__global__ __launch_bounds__(256) void k_swt_fwd_fused(const float* __restrict__ in, float* __restrict__ cA, float* __restrict__ cH,
                                                        float* __restrict__ cV, float* __restrict__ cD, int Nr, int Nc, int fct, int M,
                                                        TapsLH f, int knob_xcd, const void* tbl)
{
    if (tbl) {  // batched launch (pdwt_batch2d_* on SWT instances): gridDim.z = image, five pointers per image (in, cA, cH, cV, cD)
        typedef const unsigned long long __attribute__((address_space(4))) * tbl_t;
        const tbl_t q = (tbl_t)(const unsigned long long*)tbl + 5 * (size_t)blockIdx.z;
        in = (const float*)q[0];
        cA = (float*)q[1];
        cH = (float*)q[2];
        cV = (float*)q[3];
        cD = (float*)q[4];
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* const smem = reinterpret_cast<float*>(smem_raw);
    constexpr int C = HLEN / 2 - 1;
    const int tid = threadIdx.x;
    // XCD-aware tile order (the dispatcher deals consecutive workgroups round-robin over the 8 XCDs): every XCD gets a contiguous
    // run of the tile-major order, so the tiles of one row chunk -- whose staged rows overlap by the (hlen-1)*f halo columns -- share
    // an L2
    int bx, by;
    {
        const int T = gridDim.x * gridDim.y, w = blockIdx.y * gridDim.x + blockIdx.x;
        const int xq = w & 7, per = T >> 3, rem = T & 7;
        const int Lw = knob_xcd ? xq * per + min(xq, rem) + (w >> 3) : w;
        bx = Lw % (int)gridDim.x;
        by = Lw / (int)gridDim.x;
    }
    const int rho = by % fct;
    const int m0 = (by / fct) * M;
    const int Mc = Nr / fct;  // rows of one residue class
    const int nout = min(M, Mc - m0);
    if (nout <= 0) return;
    const int x0 = bx * kSwtTile;
    const int HLc = ((C * fct + 3) >> 2) << 2, HRc = (((HLEN - 1 - C) * fct + 3) >> 2) << 2;
    const int PW = HLc + kSwtTile + HRc;  // staged floats per row
    const int nst = PW >> 2;              // 16-byte chunks per staged row (<= 512: checked by the dispatcher)
    const int xs = x0 - HLc;              // global column of LDS index 0 (a multiple of 4, may be negative)
    const int xg = x0 + 4 * tid;
    const bool active = xg < Nc;
    const int nin = nout + HLEN - 1;  // class-local input rows m0-C .. m0+nout-1+(HLEN-1-C)

    // staging: chunk k of a row lives at global columns wrap(xs + 4k): never straddles the wrap (Nc % 4 == 0)
    const int k0 = min(tid, nst - 1), k1 = min(tid + 256, nst - 1);
    const int gc0 = wrapi(xs + 4 * k0, Nc), gc1 = wrapi(xs + 4 * k1, Nc);
    auto row_of = [&](int r) { return (size_t)SWTF_LD_ROW(rho + fct * wrapi(m0 - C + min(r, nin - 1), Mc)) * Nc; };
    // The row registers are loaded and waited for by hand (stream_dev.hpp).  Left to hipcc, the wait in front of the LDS write of row
    // r+1 is `s_waitcnt vmcnt(0)`: loads and stores share the in-order counter, the four stores of row r are younger than the two
    // loads, and the compiler does not count past stores -- every row step then waited for its own stores to reach memory (2 us per
    // step and workgroup at C3).  Counted: vmcnt(4) when the previous row stored, vmcnt(0) otherwise.
    const unsigned vo0 = (unsigned)gc0 * 4u, vo1 = (unsigned)gc1 * 4u, vox = (unsigned)(active ? xg : 0) * 4u;
    const lanemask_t amask = __ballot(active);
    const bool wstore = amask != 0;  // (a wave without a single output column only stages)
    v4f pre0 = {0.f, 0.f, 0.f, 0.f}, pre1 = {0.f, 0.f, 0.f, 0.f};
    {
        const float* p = in + row_of(0);
        asm_load_s(pre0, p, vo0);
        asm_load_s(pre1, p, vo1);
    }

    v2f ring[HLEN][4];  // (lo,hi) of the thread's 4 columns for the last HLEN rows of the class

    for (int rb = 0; rb < nin; rb += HLEN) {
        static_for<HLEN>([&](auto U) {
            constexpr int u = decltype(U)::value;
            const int r = rb + u;
            if (r < nin) {  // uniform
                float* const buf = smem + ((u & 1) ? PW : 0);  // (rb is a multiple of HLEN, which is even: r & 1 == u & 1)
                asm_wait2_sel<4>(SWTF_COUNTED && wstore && r > HLEN - 1, pre0, pre1);  // (row r-1 issued its four stores after these two loads)
                reinterpret_cast<v4f*>(buf)[k0] = pre0;
                reinterpret_cast<v4f*>(buf)[k1] = pre1;
                {  // next row's chunks fly while this one is transformed (clamped at the end: harmless re-read)
                    const float* p = in + row_of(r + 1);
                    asm_load_s(pre0, p, vo0);
                    asm_load_s(pre1, p, vo1);
                }
                swtf_barrier();
                // ---- row pass: (lo,hi)[q] = sum_j x[4 tid + q + (j - C) f] * (L,H)[HLEN-1-j] ----
                v2f acc[4];
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = v2f{0.f, 0.f};
                if constexpr (FSEL == 0) {
                    int woff = 4 * tid;  // HLc == C*f here; laundered per row (see k_swt_inv_fused4)
                    asm("" : "+v"(woff) : "s"(r));
                    const float* w0 = buf + woff;
                    static_for<HLEN>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        const v4f t = *reinterpret_cast<const v4f*>(w0 + j * fct);
                        const v2f tp = f.t[HLEN - 1 - j];
#pragma unroll
                        for (int q = 0; q < 4; q++) acc[q] = pk_fma(splat(t[q]), tp, acc[q]);
                    });
                } else {
                    constexpr int PAD = (((C * FSEL + 3) >> 2) << 2) - C * FSEL;      // window start inside its first chunk
                    constexpr int NCH = (PAD + 4 + (HLEN - 1) * FSEL + 3) / 4;          // aligned chunks covering the window
                    float w[NCH * 4];
#pragma unroll
                    for (int k = 0; k < NCH; k++) {
                        const v4f t = reinterpret_cast<const v4f*>(buf + 4 * tid)[k];
#pragma unroll
                        for (int q = 0; q < 4; q++) w[4 * k + q] = t[q];
                    }
                    static_for<HLEN>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        const v2f tp = f.t[HLEN - 1 - j];
#pragma unroll
                        for (int q = 0; q < 4; q++) acc[q] = pk_fma(splat(w[PAD + q + j * FSEL]), tp, acc[q]);
                    });
                }
#pragma unroll
                for (int q = 0; q < 4; q++) ring[u][q] = acc[q];
                // ---- column pass once the window r-HLEN+1 .. r is complete: output row m0 + r - (HLEN-1) of the class ----
                if (r >= HLEN - 1) {
                    v2f ah[4], vd[4];  // (A,H) from lo, (V,D) from hi
#pragma unroll
                    for (int q = 0; q < 4; q++) ah[q] = vd[q] = v2f{0.f, 0.f};
                    static_for<HLEN>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        constexpr int s = (u + 1 + j) % HLEN;  // oldest row first
                        const v2f tp = f.t[HLEN - 1 - j];
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            ah[q] = pk_fma(splat(ring[s][q].x), tp, ah[q]);
                            vd[q] = pk_fma(splat(ring[s][q].y), tp, vd[q]);
                        }
                    });
                    if (wstore) {  // uniform; lanes without an output column are masked through EXEC, the instruction still counts
                        const size_t o = (size_t)SWTF_ST_ROW(rho + fct * (m0 + r - (HLEN - 1))) * Nc;
                        // the three detail bands are final results nobody reads before the inverse: non-temporal stores keep them from
                        // displacing the approximation (which the next level reads back) -- forward levels of C3 356 -> 328 us; the
                        // approximation itself stored non-temporally loses all of that again, and so do nt loads / stores in the inverse
                        asm_store_sm(cA + o, vox, v4f{ah[0].x, ah[1].x, ah[2].x, ah[3].x}, amask);
                        asm_store_sm_nt(cH + o, vox, v4f{ah[0].y, ah[1].y, ah[2].y, ah[3].y}, amask);
                        asm_store_sm_nt(cV + o, vox, v4f{vd[0].x, vd[1].x, vd[2].x, vd[3].x}, amask);
                        asm_store_sm_nt(cD + o, vox, v4f{vd[0].y, vd[1].y, vd[2].y, vd[3].y}, amask);
                    }
                }
            }
        });
    }
    asm_wait2<0>(pre0, pre1);  // (the clamped prefetch of the last step)
}

#endif
#if PDWT_SWTF_PART == 2 || PDWT_SWTF_PART == 5
// -------------------------------------------------------------------------------------------------
// inverse level in one launch.  The reference synthesises columns first, then rows (src/separable.cu:553-626);
// that order would need the column results at the halo COLUMNS of the tile.  The two 1-D operators commute, so
// here every staged row goes through the ROW synthesis first,
//     u1 = IL_x(A) + IH_x(V),   u2 = IL_x(H) + IH_x(D)        (A,H: row-low-pass branch; V,D: row-high-pass branch)
// (u1,u2) enter the register ring and the COLUMN synthesis out = IL_y(u1) + IH_y(u2) emits one image row per
// input row -- the mirror image of the forward kernel.  Same taps, same products, a different summation
// order than the two-pass kernels: equal to them within a few ulp (tests: 1e-5 relative, like every SWT inverse
// comparison -- the reference itself halves each product where this build halves the taps once).
// -------------------------------------------------------------------------------------------------
// 4 columns per thread, 16-byte accesses (a 2-column variant measured slower: 660 vs 559 us for the 5 levels of C3)
template <int HLEN, int FSEL>
__global__ __launch_bounds__(256) void k_swt_inv_fused4(const float* __restrict__ cA, const float* __restrict__ cH, const float* __restrict__ cV,
                                                        const float* __restrict__ cD, float* __restrict__ out, int Nr, int Nc, int fct, int M,
                                                        Taps2<float> f, int knob_xcd, int alt, const void* tbl)
{
    if (tbl) {  // batched launch: (cA, cH, cV, cD, out) of image blockIdx.z
        typedef const unsigned long long __attribute__((address_space(4))) * tbl_t;
        const tbl_t q = (tbl_t)(const unsigned long long*)tbl + 5 * (size_t)blockIdx.z;
        cA = (const float*)q[0];
        cH = (const float*)q[1];
        cV = (const float*)q[2];
        cD = (const float*)q[3];
        out = (float*)q[4];
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* const smem = reinterpret_cast<float*>(smem_raw);
    constexpr int C = HLEN / 2;  // synthesis centre (A-4)
    const int tid = threadIdx.x;
    // XCD-aware tile order (the dispatcher deals consecutive workgroups round-robin over the 8 XCDs): every XCD gets a contiguous
    // run of the tile-major order, so the tiles of one row chunk -- whose staged rows overlap by the (hlen-1)*f halo columns -- share
    // an L2
    int bx, by;
    {
        const int T = gridDim.x * gridDim.y, w = blockIdx.y * gridDim.x + blockIdx.x;
        const int xq = w & 7, per = T >> 3, rem = T & 7;
        const int Lw = knob_xcd ? xq * per + min(xq, rem) + (w >> 3) : w;
        bx = Lw % (int)gridDim.x;
        by = Lw / (int)gridDim.x;
    }
    SWTF_INV_CHUNK(fct)
    const int x0 = bx * kSwtTile;
    const int HLc = ((C * fct + 3) >> 2) << 2, HRc = (((HLEN - 1 - C) * fct + 3) >> 2) << 2;
    // WP (tap spacing 1 and 2): every WAVE stages the 256 columns it synthesises plus their halo into a region of its own, so no wave reads
    // what another wave wrote and the row needs no workgroup barrier (DS operations of one wave run in order); the halo (26 f columns per wave
    // instead of per workgroup) is 10-20 % more staging at these spacings and would be 1.4-2.6x at spacing 4-16, which keep the shared rows
    constexpr bool WP = SWTF_WAVE_PRIVATE && FSEL != 0;
    const int wv = tid >> 6, sid = WP ? (tid & 63) : tid;
    const int PW = HLc + (WP ? 256 : kSwtTile) + HRc;
    const int nst = PW >> 2;  // 16-byte chunks per staged row (<= 512)
    const int xs = x0 + (WP ? 256 * wv : 0) - HLc;
    const int xg = x0 + 4 * tid;
    const bool active = xg < Nc;
    const int nin = nout + HLEN - 1;
    const int k0 = min(sid, nst - 1), k1 = min(sid + (WP ? 64 : 256), nst - 1);
    const int gc0 = wrapi(xs + 4 * k0, Nc), gc1 = wrapi(xs + 4 * k1, Nc);
    SWTF_INV_WALK(fct)
    const float* const band[4] = {cA, cV, cH, cD};  // staging order: (A,V) feed u1, (H,D) feed u2
    // row registers loaded and waited for by hand (see k_swt_fwd_fused): vmcnt(1) when a store was issued behind the eight loads
    const unsigned vo0 = (unsigned)gc0 * 4u, vo1 = (unsigned)gc1 * 4u, vox = (unsigned)(active ? xg : 0) * 4u;
    const lanemask_t amask = __ballot(active);
    const bool wstore = amask != 0;
    v4f pre[4][2];
    {
        const size_t o = row_of(0);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            pre[b][0] = pre[b][1] = v4f{0.f, 0.f, 0.f, 0.f};
            asm_load_s(pre[b][0], band[b] + o, vo0);
            asm_load_s(pre[b][1], band[b] + o, vo1);
        }
    }
    auto wait_rows = [&](bool stored) { asm_wait8_sel<1>(stored, pre[0][0], pre[0][1], pre[1][0], pre[1][1], pre[2][0], pre[2][1], pre[3][0], pre[3][1]); };
    v2f ru1[HLEN][2], ru2[HLEN][2];  // ring: (u1, u2) of the thread's 4 columns (two packed pairs each)

    for (int rb = 0; rb < nin; rb += HLEN) {
        static_for<HLEN>([&](auto U) {
            constexpr int u = decltype(U)::value;
            const int r = rb + u;
            if (r < nin) {
                float* const buf = smem + (WP ? wv * 8 * PW : 0) + ((u & 1) ? 4 * PW : 0);
                wait_rows(SWTF_COUNTED && wstore && r > HLEN - 1);  // (row r-1 stored its image row after these loads were issued)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    reinterpret_cast<v4f*>(buf + b * PW)[k0] = pre[b][0];
                    reinterpret_cast<v4f*>(buf + b * PW)[k1] = pre[b][1];
                }
                {
                    const size_t o = row_of(r + 1);
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        asm_load_s(pre[b][0], band[b] + o, vo0);
                        asm_load_s(pre[b][1], band[b] + o, vo1);
                    }
                }
                if constexpr (!WP) swtf_barrier();
                // ---- row synthesis: s[b] = sum_j band_b[x + (j - C) f] * tap_b[HLEN-1-j], the column pair packed ----
                v2f sacc[4][2];
                static_for<4>([&](auto B) {
                    constexpr int b = decltype(B)::value;
                    sacc[b][0] = sacc[b][1] = v2f{0.f, 0.f};
                    // Laundered per row: otherwise the 4*HLEN tap addresses (w0 + j*fct, fct a run-time value) are hoisted out of the
                    // row loop as 2 x 56 loop-invariant registers (292 VGPRs).  On the OFFSET, not the pointer (a laundered LDS
                    // pointer loses its address space: every ds_read becomes a flat_load), and NOT volatile (a volatile asm is
                    // a barrier for every memory operation around it) but fed the row index so it cannot be hoisted or merged.
                    int woff = b * PW + 4 * sid;
                    asm("" : "+v"(woff) : "s"(r));
                    const float* w0 = buf + woff;
                    if constexpr (FSEL == 0) {
                        static_for<HLEN>([&](auto J) {
                            constexpr int j = decltype(J)::value;
                            const v4f t = *reinterpret_cast<const v4f*>(w0 + j * fct);
                            const v2f tp = splat((b & 1) ? f.b[HLEN - 1 - j] : f.a[HLEN - 1 - j]);
                            sacc[b][0] = pk_fma(v2f{t[0], t[1]}, tp, sacc[b][0]);
                            sacc[b][1] = pk_fma(v2f{t[2], t[3]}, tp, sacc[b][1]);
                        });
                    } else {
                        constexpr int PAD = (((C * FSEL + 3) >> 2) << 2) - C * FSEL;
                        constexpr int NCH = (PAD + 4 + (HLEN - 1) * FSEL + 3) / 4;
                        float w[NCH * 4];
#pragma unroll
                        for (int k = 0; k < NCH; k++) {
                            const v4f t = reinterpret_cast<const v4f*>(w0)[k];
#pragma unroll
                            for (int q = 0; q < 4; q++) w[4 * k + q] = t[q];
                        }
                        static_for<HLEN>([&](auto J) {
                            constexpr int j = decltype(J)::value;
                            const v2f tp = splat((b & 1) ? f.b[HLEN - 1 - j] : f.a[HLEN - 1 - j]);
                            sacc[b][0] = pk_fma(v2f{w[PAD + j * FSEL], w[PAD + 1 + j * FSEL]}, tp, sacc[b][0]);
                            sacc[b][1] = pk_fma(v2f{w[PAD + 2 + j * FSEL], w[PAD + 3 + j * FSEL]}, tp, sacc[b][1]);
                        });
                    }
                });
                ru1[u][0] = sacc[0][0] + sacc[1][0];  // band[]: 0 = A (IL), 1 = V (IH), 2 = H (IL), 3 = D (IH)
                ru1[u][1] = sacc[0][1] + sacc[1][1];
                ru2[u][0] = sacc[2][0] + sacc[3][0];
                ru2[u][1] = sacc[2][1] + sacc[3][1];
                // ---- column synthesis: out = IL_y(u1) + IH_y(u2) over the window r-HLEN+1 .. r ----
                if (r >= HLEN - 1) {
                    v2f o1[2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}}, o2[2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}};
                    static_for<HLEN>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        constexpr int s = (u + 1 + j) % HLEN;
                        o1[0] = pk_fma_sbcast<j & 1, false>(ru1[s][0], cpa[j >> 1], o1[0]);
                        o1[1] = pk_fma_sbcast<j & 1, false>(ru1[s][1], cpa[j >> 1], o1[1]);
                        o2[0] = pk_fma_sbcast<j & 1, false>(ru2[s][0], cpb[j >> 1], o2[0]);
                        o2[1] = pk_fma_sbcast<j & 1, false>(ru2[s][1], cpb[j >> 1], o2[1]);
                    });
                    if (wstore) {
                        const v2f a0 = o1[0] + o2[0], a1 = o1[1] + o2[1];
                        asm_store_sm(out + (size_t)SWTF_ST_ROW(rho + fct * (ob0 + rst * r)) * Nc, vox, (v4f{a0.x, a0.y, a1.x, a1.y}), amask);
                    }
                }
            }
        });
    }
    wait_rows(false);  // (the clamped prefetch of the last step)
}


#endif
#if PDWT_SWTF_PART == 3
// -------------------------------------------------------------------------------------------------
// The same inverse level for tap spacings F = 4, 8, 16 with the staged rows held RESIDUE-MAJOR in LDS.  In k_swt_inv_fused4 every
// tap of a dilated filter is its own 16-byte read (4 bands x 14 taps = 56 reads per thread and row: the LDS pipe is what bounds levels
// 3-5 of C3, 101 us against 85 for the levels with spacing 1 and 2).  Columns x = sigma (mod F) form F sub-rows on which the dilated row
// filter is dense: stored sub-row after sub-row, a thread that owns FOUR CONSECUTIVE samples of one sub-row reads its whole window as
// 5 aligned 16-byte chunks (20 reads instead of 56).  The staging writes scatter each loaded chunk over 4 sub-rows (4-byte writes), and
// the finished image row goes back through a residue-major LDS row (one 16-byte write, four 4-byte reads per thread) so that the
// global store is the same coalesced 16-byte store as before -- one row late, behind the next row's barrier.  Arithmetic and summation
// order per output are those of k_swt_inv_fused4: bit-identical results.
// -------------------------------------------------------------------------------------------------
template <int HLEN, int F>
__global__ __launch_bounds__(256) void k_swt_inv_fusedp(const float* __restrict__ cA, const float* __restrict__ cH, const float* __restrict__ cV,
                                                        const float* __restrict__ cD, float* __restrict__ out, int Nr, int Nc, int M,
                                                        Taps2<float> f, int knob_xcd, int alt, const void* tbl)
{
    if (tbl) {  // batched launch: (cA, cH, cV, cD, out) of image blockIdx.z
        typedef const unsigned long long __attribute__((address_space(4))) * tbl_t;
        const tbl_t q = (tbl_t)(const unsigned long long*)tbl + 5 * (size_t)blockIdx.z;
        cA = (const float*)q[0];
        cH = (const float*)q[1];
        cV = (const float*)q[2];
        cD = (const float*)q[3];
        out = (float*)q[4];
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* const smem = reinterpret_cast<float*>(smem_raw);
    constexpr int C = HLEN / 2;                                  // synthesis centre (A-4)
    constexpr int fct = F;
    constexpr int NPR = kSwtTile / F;                            // outputs of a tile per residue class
    constexpr int BL = (NPR + HLEN - 1 + 3) & ~3;                // samples of a sub-row (window of the last output included), 16-byte multiple
    constexpr int ROW = F * BL;                                  // floats per staged row and band
    constexpr int OBL = NPR;                                     // output row: residue-major, NPR floats per class
    constexpr int HLc = C * F, HRc = (HLEN - 1 - C) * F;         // (F is a multiple of 4: no rounding)
    constexpr int PW = HLc + kSwtTile + HRc;
    constexpr int nst = PW >> 2;                                 // 16-byte chunks per staged row (<= 512)
    float* const obuf = smem + 2 * 4 * ROW;                      // two output rows
    const int tid = threadIdx.x;
    int bx, by;
    {
        const int T = gridDim.x * gridDim.y, w = blockIdx.y * gridDim.x + blockIdx.x;
        const int xq = w & 7, per = T >> 3, rem = T & 7;
        const int Lw = knob_xcd ? xq * per + min(xq, rem) + (w >> 3) : w;
        bx = Lw % (int)gridDim.x;
        by = Lw / (int)gridDim.x;
    }
    SWTF_INV_CHUNK(fct)
    const int x0 = bx * kSwtTile;
    const int xs = x0 - HLc;
    const int xg = x0 + 4 * tid;
    const bool active = xg < Nc;
    const int nin = nout + HLEN - 1;
    // staging: chunk k holds staged positions 4k .. 4k+3 = sub-rows (4k % F) + e, index 4k / F
    const int k0 = min(tid, nst - 1), k1 = min(tid + 256, nst - 1);
    const int gc0 = wrapi(xs + 4 * k0, Nc), gc1 = wrapi(xs + 4 * k1, Nc);
    const int so0 = ((4 * k0) % F) * BL + (4 * k0) / F, so1 = ((4 * k1) % F) * BL + (4 * k1) / F;
    // outputs: thread -> (sub-row sigma, four consecutive samples 4m .. 4m+3 of it) = tile columns sigma + F (4m + e)
    const int sigma = tid / (NPR / 4), m4 = 4 * (tid % (NPR / 4));
    const int woff0 = sigma * BL + m4;        // window of sample n starts at index n of the sub-row (position = n + C in units of F, minus C)
    const int ooff = sigma * OBL + m4;        // where the thread's four results go in the output row
    // the coalesced store of the row: thread tid stores tile columns 4 tid .. 4 tid + 3 = sub-rows (4 tid % F) + e, index 4 tid / F
    const int roff = ((4 * tid) % F) * OBL + (4 * tid) / F;
    SWTF_INV_WALK(fct)
    const float* const band[4] = {cA, cV, cH, cD};  // staging order: (A,V) feed u1, (H,D) feed u2
    // row registers loaded and waited for by hand (see k_swt_fwd_fused): vmcnt(1) when a store was issued behind the eight loads
    const unsigned vo0 = (unsigned)gc0 * 4u, vo1 = (unsigned)gc1 * 4u, vox = (unsigned)(active ? xg : 0) * 4u;
    const lanemask_t amask = __ballot(active);
    const bool wstore = amask != 0;
    v4f pre[4][2];
    {
        const size_t o = row_of(0);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            pre[b][0] = pre[b][1] = v4f{0.f, 0.f, 0.f, 0.f};
            asm_load_s(pre[b][0], band[b] + o, vo0);
            asm_load_s(pre[b][1], band[b] + o, vo1);
        }
    }
    auto wait_rows = [&](bool stored) { asm_wait8_sel<1>(stored, pre[0][0], pre[0][1], pre[1][0], pre[1][1], pre[2][0], pre[2][1], pre[3][0], pre[3][1]); };
    v2f ru1[HLEN][2], ru2[HLEN][2];  // ring: (u1, u2) of the thread's 4 outputs (two packed pairs each)
    int pending = -1;                // class row whose image row waits in obuf[(pending_slot)]
    int pslot = 0;

    for (int rb = 0; rb < nin; rb += HLEN) {
        static_for<HLEN>([&](auto U) __attribute__((always_inline)) {
            constexpr int u = decltype(U)::value;
            const int r = rb + u;
            if (r < nin) {
                float* const buf = smem + ((u & 1) ? 4 * ROW : 0);
                wait_rows(SWTF_COUNTED && wstore && r > HLEN);  // (step r-1 stored the row finished in step r-2, after these loads were issued)
#pragma unroll
                for (int b = 0; b < 4; b++) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        buf[b * ROW + so0 + e * BL] = pre[b][0][e];
                        buf[b * ROW + so1 + e * BL] = pre[b][1][e];
                    }
                }
                {
                    const size_t o = row_of(r + 1);
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        asm_load_s(pre[b][0], band[b] + o, vo0);
                        asm_load_s(pre[b][1], band[b] + o, vo1);
                    }
                }
                swtf_barrier();
                // the image row finished one step ago: out of the residue-major row, into memory (coalesced)
                if (pending >= 0) {
                    const float* ob = obuf + pslot * kSwtTile + roff;
                    const v4f v = v4f{ob[0], ob[OBL], ob[2 * OBL], ob[3 * OBL]};
                    if (wstore) asm_store_sm(out + (size_t)SWTF_ST_ROW(rho + fct * pending) * Nc, vox, v, amask);
                    pending = -1;
                }
                // ---- row synthesis on the thread's sub-row: s[b][e] = sum_j sub_b[4m + e + j] * tap_b[HLEN-1-j] ----
                v2f sacc[4][2];
                static_for<4>([&](auto B) __attribute__((always_inline)) {
                    constexpr int b = decltype(B)::value;
                    sacc[b][0] = sacc[b][1] = v2f{0.f, 0.f};
                    int woff = b * ROW + woff0;
                    asm("" : "+v"(woff) : "s"(r));  // (see k_swt_inv_fused4: keeps the window addresses out of loop-invariant registers)
                    const float* w0 = buf + woff;
                    constexpr int NCH = (4 + HLEN - 1 + 3) / 4;
                    float w[NCH * 4];
#pragma unroll
                    for (int k = 0; k < NCH; k++) {
                        const v4f t = reinterpret_cast<const v4f*>(w0)[k];
#pragma unroll
                        for (int q = 0; q < 4; q++) w[4 * k + q] = t[q];
                    }
                    static_for<HLEN>([&](auto J) __attribute__((always_inline)) {
                        constexpr int j = decltype(J)::value;
                        const v2f tp = splat((b & 1) ? f.b[HLEN - 1 - j] : f.a[HLEN - 1 - j]);
                        sacc[b][0] = pk_fma(v2f{w[j], w[1 + j]}, tp, sacc[b][0]);
                        sacc[b][1] = pk_fma(v2f{w[2 + j], w[3 + j]}, tp, sacc[b][1]);
                    });
                });
                ru1[u][0] = sacc[0][0] + sacc[1][0];  // band[]: 0 = A (IL), 1 = V (IH), 2 = H (IL), 3 = D (IH)
                ru1[u][1] = sacc[0][1] + sacc[1][1];
                ru2[u][0] = sacc[2][0] + sacc[3][0];
                ru2[u][1] = sacc[2][1] + sacc[3][1];
                // ---- column synthesis: out = IL_y(u1) + IH_y(u2) over the window r-HLEN+1 .. r ----
                if (r >= HLEN - 1) {
                    v2f o1[2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}}, o2[2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}};
                    static_for<HLEN>([&](auto J) __attribute__((always_inline)) {
                        constexpr int j = decltype(J)::value;
                        constexpr int s = (u + 1 + j) % HLEN;
                        o1[0] = pk_fma_sbcast<j & 1, false>(ru1[s][0], cpa[j >> 1], o1[0]);
                        o1[1] = pk_fma_sbcast<j & 1, false>(ru1[s][1], cpa[j >> 1], o1[1]);
                        o2[0] = pk_fma_sbcast<j & 1, false>(ru2[s][0], cpb[j >> 1], o2[0]);
                        o2[1] = pk_fma_sbcast<j & 1, false>(ru2[s][1], cpb[j >> 1], o2[1]);
                    });
                    const v2f a0 = o1[0] + o2[0], a1 = o1[1] + o2[1];
                    pslot = u & 1;
                    *reinterpret_cast<v4f*>(obuf + pslot * kSwtTile + ooff) = v4f{a0.x, a0.y, a1.x, a1.y};
                    pending = ob0 + rst * r;
                }
            }
        });
    }
    if (pending >= 0) {  // the last row
        swtf_barrier();
        const float* ob = obuf + pslot * kSwtTile + roff;
        const v4f v = v4f{ob[0], ob[OBL], ob[2 * OBL], ob[3 * OBL]};
        if (wstore) asm_store_sm(out + (size_t)SWTF_ST_ROW(rho + fct * pending) * Nc, vox, v, amask);
    }
    wait_rows(false);  // (the clamped prefetch of the last step)
}

#endif

#define PDWT_CHECK_LAUNCH() PDWT_HIP_TRY(hipGetLastError())
#ifndef PDWT_SWTF_HLENS  // (experiment builds restrict the list: tools/build_variant.sh ... '-DPDWT_SWTF_HLENS(X)=X(14)')
#if PDWT_SWTF_PART == 1 || PDWT_SWTF_PART == 2
#define PDWT_SWTF_HLENS(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16)
#elif PDWT_SWTF_PART == 3
#define PDWT_SWTF_HLENS(X) X(8) X(10) X(12) X(14) X(16)  // (shorter banks: few window reads to save)
#else
#define PDWT_SWTF_HLENS(X) X(18) X(20)  // ring of 8*hlen registers: 1-2 waves per SIMD, still 3x the two-pass kernels
#endif
#endif
// d_tbl != NULL: a batch of nimg images in one launch (gridDim.z = image; five device pointers per image, the pointer arguments are ignored)
int swt_fwd_fused_long_f32(const float* in, float* cA, float* cH, float* cV, float* cD, int Nr, int Nc, int hlen, int fct, const Taps2<float>& f,
                           const void* d_tbl, int nimg);
int swt_inv_fused_long_f32(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int hlen, int fct,
                           const Taps2<float>& f, const void* d_tbl, int nimg);
int swt_inv_fusedp_f32(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int hlen, int fct, int M,
                       const Taps2<float>& f, const void* d_tbl, int nimg);
// banks of 22 ... 40 taps: two columns per thread, zero-padded to 24 / 32 / 40 taps (swt_fused_l2.inc)
int swt_fwd_fused_l2_f32(const float* in, float* cA, float* cH, float* cV, float* cD, int Nr, int Nc, int hlen, int fct, const Taps2<float>& f,
                         const void* d_tbl, int nimg);
int swt_inv_fused_l2_f32(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int hlen, int fct,
                         const Taps2<float>& f, const void* d_tbl, int nimg);

#if PDWT_SWTF_PART == 1 || PDWT_SWTF_PART == 4
template <int HLEN>
static int launch_swt_fwd(const float* in, float* cA, float* cH, float* cV, float* cD, int Nr, int Nc, int fct, const Taps2<float>& f2, const void* d_tbl,
                          int nimg)
{
    constexpr int C = HLEN / 2 - 1;
    TapsLH f;
    for (int k = 0; k < PDWT_MAX_FILTER_WIDTH; k++) f.t[k] = v2f{f2.a[k], f2.b[k]};
    const int HLc = ((C * fct + 3) >> 2) << 2, HRc = (((HLEN - 1 - C) * fct + 3) >> 2) << 2;
    const int PW = HLc + kSwtTile + HRc;
    if (PW / 4 > 512 || PW - kSwtTile > Nc) return 1;  // two staging chunks per thread; halo shorter than a row
    const size_t lds = 2 * (size_t)PW * sizeof(float) + 64;  // (+ slack: the last thread's window read is rounded up to 16 bytes)
    const int Mc = Nr / fct;
    // rows of a class per workgroup: as many workgroups as are resident at once (three per CU at <= 168 VGPRs: 768), not one more
    // (a fourth on some CUs runs alone afterwards: M = 21 -> 784 workgroups, 86 us per level at 4096^2 db7; M = 22 -> 748: 75;
    // M = 24 -> 684: 78; 32: 80; 64: 100; 128: 140): shorter chunks pay HLEN-1 warm-up rows each, taller ones leave too few
    // workgroups to overlap the per-row barrier
    const int tiles = idiv_up(Nc, kSwtTile);
    int M = knob(KN_SWTF_M);
    if (M <= 0) {  // (a batch shares the resident workgroups between its images)
        M = (int)(((long long)Mc * fct * tiles * nimg + 767) / 768);
        if (M < HLEN) M = HLEN;
    }
    if (M > Mc) M = Mc;
    dim3 grid(tiles, fct * idiv_up(Mc, M), nimg);
    stat_hit(ST_SWTF_FWD);
    KTimer kt(K_SWT_ANA_COLS, true);
    if (fct == 1) PDWT_LAUNCH_KT(kt, (k_swt_fwd_fused<HLEN, 1>), grid, dim3(256), lds, in, cA, cH, cV, cD, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), d_tbl);
    else if (fct == 2) PDWT_LAUNCH_KT(kt, (k_swt_fwd_fused<HLEN, 2>), grid, dim3(256), lds, in, cA, cH, cV, cD, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), d_tbl);
    else PDWT_LAUNCH_KT(kt, (k_swt_fwd_fused<HLEN, 0>), grid, dim3(256), lds, in, cA, cH, cV, cD, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), d_tbl);
    PDWT_CHECK_LAUNCH();
    return PDWT_OK;
}

#if PDWT_SWTF_PART == 1
int swt_fwd_fused_f32(const float* in, float* cA, float* cH, float* cV, float* cD, int Nr, int Nc, int hlen, int fct, const Taps2<float>& f,
                      const void* d_tbl, int nimg)
{
    if (knob(KN_SWTF) != 1 || !counted_waits_ok()) return 1;  // (row registers waited for by hand: selfcheck.hip)
    if ((Nc & 3) || Nc < 64 || (Nr % fct) != 0 || Nr / fct < 2 * hlen) return 1;
    if (!d_tbl) {  // (a batch: alignment and aliasing of every image's pointers were checked when its tables were built)
        if (!al16(in) || !al16(cA) || !al16(cH) || !al16(cV) || !al16(cD)) return 1;
        if (in == cA || in == cH || in == cV || in == cD) return 1;  // one launch: the input must not be a band being written
    }
    switch (hlen) {
#define X(H) \
    case H: return launch_swt_fwd<H>(in, cA, cH, cV, cD, Nr, Nc, fct, f, d_tbl, nimg);
        PDWT_SWTF_HLENS(X)
#undef X
        default: return swt_fwd_fused_long_f32(in, cA, cH, cV, cD, Nr, Nc, hlen, fct, f, d_tbl, nimg);
    }
}
#else
int swt_fwd_fused_long_f32(const float* in, float* cA, float* cH, float* cV, float* cD, int Nr, int Nc, int hlen, int fct, const Taps2<float>& f,
                           const void* d_tbl, int nimg)
{
    switch (hlen) {  // (geometry already checked by swt_fwd_fused_f32)
#define X(H) \
    case H: return launch_swt_fwd<H>(in, cA, cH, cV, cD, Nr, Nc, fct, f, d_tbl, nimg);
        PDWT_SWTF_HLENS(X)
#undef X
        default: return swt_fwd_fused_l2_f32(in, cA, cH, cV, cD, Nr, Nc, hlen, fct, f, d_tbl, nimg);
    }
}
#endif

#endif
#if PDWT_SWTF_PART == 2 || PDWT_SWTF_PART == 5
template <int HLEN>
static int launch_swt_inv4(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int fct,
                           const Taps2<float>& f, const void* d_tbl, int nimg)
{
    constexpr int C = HLEN / 2;
    const int HLc = ((C * fct + 3) >> 2) << 2, HRc = (((HLEN - 1 - C) * fct + 3) >> 2) << 2;
    const int PW = HLc + kSwtTile + HRc;
    if (PW / 4 > 512 || PW - kSwtTile > Nc) return 1;
    const bool wp = SWTF_WAVE_PRIVATE && (fct == 1 || fct == 2);  // four wave-private regions of 256 columns + halo
    const size_t lds = (wp ? 4 * 2 * 4 * (size_t)(HLc + 256 + HRc) : 2 * 4 * (size_t)PW) * sizeof(float) + 64;
    if (lds > 64 * 1024) return 1;
    const int Mc = Nr / fct;
    const int tiles = idiv_up(Nc, kSwtTile);
    int M = knob(KN_SWTF_MI);
    if (M <= 0) {
        M = (int)(((long long)Mc * fct * tiles * nimg + 511) / 512);
        if (M < HLEN) M = HLEN;
    }
    if (M > Mc) M = Mc;
    dim3 grid(tiles, fct * idiv_up(Mc, M), nimg);
#if PDWT_SWTF_PART == 2
    if ((fct == 4 || fct == 8 || fct == 16) && knob(KN_SWTF_PERM) == 1) {  // residue-major LDS rows (part 3)
        const int rc = swt_inv_fusedp_f32(cA, cH, cV, cD, out, Nr, Nc, HLEN, fct, M, f, d_tbl, nimg);
        if (rc <= 0) return rc;
    }
#endif
    stat_hit(ST_SWTF_INV);
    KTimer kt(K_SWT_SYN_COLS, true);
    if (fct == 1) PDWT_LAUNCH_KT(kt, (k_swt_inv_fused4<HLEN, 1>), grid, dim3(256), lds, cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), knob(KN_SWTF_ALT), d_tbl);
    else if (fct == 2) PDWT_LAUNCH_KT(kt, (k_swt_inv_fused4<HLEN, 2>), grid, dim3(256), lds, cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), knob(KN_SWTF_ALT), d_tbl);
    else PDWT_LAUNCH_KT(kt, (k_swt_inv_fused4<HLEN, 0>), grid, dim3(256), lds, cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), knob(KN_SWTF_ALT), d_tbl);
    PDWT_CHECK_LAUNCH();
    return PDWT_OK;
}

#if PDWT_SWTF_PART == 2
int swt_inv_fused_f32(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int hlen, int fct,
                      const Taps2<float>& f, const void* d_tbl, int nimg)
{
    if (knob(KN_SWTF) != 1 || !counted_waits_ok()) return 1;  // (row registers waited for by hand: selfcheck.hip)
    if ((Nc & 3) || Nc < 64 || (Nr % fct) != 0 || Nr / fct < 2 * hlen) return 1;
    if (!d_tbl) {
        if (!al16(out) || !al16(cA) || !al16(cH) || !al16(cV) || !al16(cD)) return 1;
        if (out == cA || out == cH || out == cV || out == cD) return 1;
    }
    switch (hlen) {
#define X(H) \
    case H: return launch_swt_inv4<H>(cA, cH, cV, cD, out, Nr, Nc, fct, f, d_tbl, nimg);
        PDWT_SWTF_HLENS(X)
#undef X
        default: return swt_inv_fused_long_f32(cA, cH, cV, cD, out, Nr, Nc, hlen, fct, f, d_tbl, nimg);
    }
}
#else
int swt_inv_fused_long_f32(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int hlen, int fct,
                           const Taps2<float>& f, const void* d_tbl, int nimg)
{
    switch (hlen) {  // (geometry already checked by swt_inv_fused_f32)
#define X(H) \
    case H: return launch_swt_inv4<H>(cA, cH, cV, cD, out, Nr, Nc, fct, f, d_tbl, nimg);
        PDWT_SWTF_HLENS(X)
#undef X
        default: return swt_inv_fused_l2_f32(cA, cH, cV, cD, out, Nr, Nc, hlen, fct, f, d_tbl, nimg);
    }
}
#endif

#endif
#if PDWT_SWTF_PART == 3
template <int HLEN>
static int launch_swt_invp(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int fct, int M,
                           const Taps2<float>& f, const void* d_tbl, int nimg)
{
    if (kSwtTile % (4 * fct) != 0) return 1;
    // F sub-rows of ((1024 / F + HLEN - 1) rounded up to 4) floats per band, two row buffers, two output rows
    const int bl = ((kSwtTile / fct + HLEN - 1) + 3) & ~3;
    const size_t ldsp = (2 * 4 * (size_t)fct * bl + 2 * kSwtTile) * sizeof(float) + 64;
    if (ldsp > 64 * 1024) return 1;
    const int Mc = Nr / fct;
    dim3 grid(idiv_up(Nc, kSwtTile), fct * idiv_up(Mc, M), nimg);
    if (fct == 4 || fct == 8 || fct == 16) stat_hit(ST_SWTF_INVP);
    KTimer kt(K_SWT_SYN_COLS, true);
    if (fct == 4) PDWT_LAUNCH_KT(kt, (k_swt_inv_fusedp<HLEN, 4>), grid, dim3(256), ldsp, cA, cH, cV, cD, out, Nr, Nc, M, f, knob(KN_SWTF_XCD), knob(KN_SWTF_ALT), d_tbl);
    else if (fct == 8) PDWT_LAUNCH_KT(kt, (k_swt_inv_fusedp<HLEN, 8>), grid, dim3(256), ldsp, cA, cH, cV, cD, out, Nr, Nc, M, f, knob(KN_SWTF_XCD), knob(KN_SWTF_ALT), d_tbl);
    else if (fct == 16) PDWT_LAUNCH_KT(kt, (k_swt_inv_fusedp<HLEN, 16>), grid, dim3(256), ldsp, cA, cH, cV, cD, out, Nr, Nc, M, f, knob(KN_SWTF_XCD), knob(KN_SWTF_ALT), d_tbl);
    else return 1;
    PDWT_CHECK_LAUNCH();
    return PDWT_OK;
}

int swt_inv_fusedp_f32(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int hlen, int fct, int M,
                       const Taps2<float>& f, const void* d_tbl, int nimg)
{
    switch (hlen) {  // (geometry and chunk height come from launch_swt_inv4)
#define X(H) \
    case H: return launch_swt_invp<H>(cA, cH, cV, cD, out, Nr, Nc, fct, M, f, d_tbl, nimg);
        PDWT_SWTF_HLENS(X)
#undef X
        default: return 1;
    }
}
#endif

}  // namespace pdwt
