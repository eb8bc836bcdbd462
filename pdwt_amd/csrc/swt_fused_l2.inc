// swt_fused_l2.inc -- one level of the 2-D stationary transform in ONE launch for float32 banks of 22 ... 40 taps.
//
// swt_fused.inc keeps the row-pass results of the last HLEN rows in a register ring of 4 columns per thread: 8 * HLEN registers, which
// stops at 20 taps (290 VGPRs) -- longer banks ran the two-pass kernels (4096^2 db16 L3 pair: 4.2 ms against 0.7 ms for 20 taps).
// The same design with TWO columns per thread (ring = 4 * HLEN registers, 512-column tiles, 8-byte accesses) carries the ring up to 40
// taps at two waves per SIMD.  Only three lengths are instantiated -- 24, 32, 40 -- and a bank of hlen taps runs the next one with
// q = (H' - hlen) / 2 zero taps at either end: analysis `out[g] = sum_j x[g - c + f j] F[hlen-1-j]`, c = (hlen/2 - 1) f, and synthesis
// `out[g] = sum_j a[g - c + f j] IL[hlen-1-j]`, c = (hlen/2) f, both keep every product where it was when the bank is padded
// symmetrically (c' = c + q f, j' = j + q), and the added terms are fma(x, 0, acc) = acc: the same result bit for bit on finite data
// (the trick of dwt_lds.hip; a NaN / Inf sample reaches up to q f more outputs per side than in the reference).
// Forward: bit-identical to the two-pass kernels and the oracle.  Inverse: rows before columns like swt_fused.inc (the operators commute);
// equal to the two-pass kernels within a few ulp (tests: 1e-5 relative).
// Reference code replaced: w_kern_forward_swt_pass1/2, w_kern_inverse_swt_pass1/2 and one iteration of their level loops
// (src/separable.cu:409-516, 553-650) at MAX_FILTER_WIDTH 40 (src/common.h:15).
#include "swt_fused.hpp"

#include "stream_dev.hpp"

namespace pdwt {

constexpr int kSwt2Tile = 512;  // columns per workgroup: 256 threads x 2

__device__ __forceinline__ void swt2_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void asm_store_sm_nt(float* sbase, unsigned voff, v2f d, lanemask_t mask)
{
    lanemask_t saved;
    asm volatile("s_and_saveexec_b64 %0, %4\n\tglobal_store_dwordx2 %1, %2, %3 nt\n\ts_mov_b64 exec, %0"
                 : "=&s"(saved) : "v"(voff), "v"(d), "s"(sbase), "s"(mask) : "memory", "scc");
}
// XCD-aware tile order (cf. swt_fused.inc): every XCD gets a contiguous run of the tile-major order
__device__ __forceinline__ void swt2_tile(int knob_xcd, int& bx, int& by)
{
    const int T = gridDim.x * gridDim.y, w = blockIdx.y * gridDim.x + blockIdx.x;
    const int xq = w & 7, per = T >> 3, rem = T & 7;
    const int Lw = knob_xcd ? xq * per + min(xq, rem) + (w >> 3) : w;
    bx = Lw % (int)gridDim.x;
    by = Lw / (int)gridDim.x;
}

#if PDWT_SWTL2_PART == 1
// WIN = true (tap spacing 1): the row-pass window is one run of aligned 8-byte reads; false (even spacings): one 8-byte read per tap
template <int HLEN, bool WIN>
__global__ __launch_bounds__(256, 2) void k_swt_fwd_fused2(const float* __restrict__ in, float* __restrict__ cA, float* __restrict__ cH,
                                                            float* __restrict__ cV, float* __restrict__ cD, int Nr, int Nc, int fct, int M,
                                                            TapsLH f, int knob_xcd, const void* tbl)
{
    if (tbl) {  // batched launch: gridDim.z = image, five pointers per image (in, cA, cH, cV, cD)
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
    int bx, by;
    swt2_tile(knob_xcd, bx, by);
    const int rho = by % fct;
    const int m0 = (by / fct) * M;
    const int Mc = Nr / fct;  // rows of one residue class
    const int nout = min(M, Mc - m0);
    if (nout <= 0) return;
    const int x0 = bx * kSwt2Tile;
    const int HLc = ((C * fct + 3) >> 2) << 2, HRc = (((HLEN - 1 - C) * fct + 3) >> 2) << 2;
    const int PW = HLc + kSwt2Tile + HRc;  // staged floats per row
    const int nst = PW >> 2;               // 16-byte chunks per staged row (<= 512: checked by the dispatcher)
    const int xs = x0 - HLc;               // global column of LDS index 0 (a multiple of 4, may be negative)
    const int xg = x0 + 2 * tid;
    const bool active = xg < Nc;
    const int nin = nout + HLEN - 1;       // class-local input rows m0-C .. m0+nout-1+(HLEN-1-C)
    const int k0 = min(tid, nst - 1), k1 = min(tid + 256, nst - 1);
    const int gc0 = wrapi(xs + 4 * k0, Nc), gc1 = wrapi(xs + 4 * k1, Nc);
    auto row_of = [&](int r) { return (size_t)(rho + fct * wrapi(m0 - C + min(r, nin - 1), Mc)) * Nc; };
    const unsigned vo0 = (unsigned)gc0 * 4u, vo1 = (unsigned)gc1 * 4u, vox = (unsigned)(active ? xg : 0) * 4u;
    const lanemask_t amask = __ballot(active);
    const bool wstore = amask != 0;  // (a wave without a single output column only stages)
    v4f pre0 = {0.f, 0.f, 0.f, 0.f}, pre1 = {0.f, 0.f, 0.f, 0.f};
    {
        const float* p = in + row_of(0);
        asm_load_s(pre0, p, vo0);
        asm_load_s(pre1, p, vo1);
    }
    v2f ring[HLEN][2];  // (lo, hi) of the thread's 2 columns for the last HLEN rows of the class
    const int pad = HLc - C * fct;  // window start inside the staged row (0 .. 3; even for even spacings)

    for (int rb = 0; rb < nin; rb += HLEN) {
        static_for<HLEN>([&](auto U) {
            constexpr int u = decltype(U)::value;
            const int r = rb + u;
            if (r < nin) {  // uniform
                float* const buf = smem + ((u & 1) ? PW : 0);
                asm_wait2_sel<4>(wstore && r > HLEN - 1, pre0, pre1);  // (row r-1 issued its four stores after these two loads)
                reinterpret_cast<v4f*>(buf)[k0] = pre0;
                reinterpret_cast<v4f*>(buf)[k1] = pre1;
                {
                    const float* p = in + row_of(r + 1);
                    asm_load_s(pre0, p, vo0);
                    asm_load_s(pre1, p, vo1);
                }
                swt2_barrier();
                // ---- row pass: (lo, hi)[q] = sum_j x[2 tid + q + (j - C) f] * (L, H)[HLEN-1-j] ----
                v2f acc[2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}};
                int woff = 2 * tid;  // laundered per row: otherwise the tap addresses are hoisted out of the row loop (cf. swt_fused.inc)
                asm("" : "+v"(woff) : "s"(r));
                if constexpr (WIN) {
                    constexpr int PAD = (((C + 3) >> 2) << 2) - C;   // fct == 1
                    constexpr int NCH = (PAD + 2 + (HLEN - 1) + 1) / 2;  // aligned 8-byte chunks covering the window
                    float w[NCH * 2];
#pragma unroll
                    for (int k = 0; k < NCH; k++) {
                        const v2f t = reinterpret_cast<const v2f*>(buf + woff)[k];
                        w[2 * k] = t.x;
                        w[2 * k + 1] = t.y;
                    }
                    static_for<HLEN>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        const v2f tp = f.t[HLEN - 1 - j];
                        acc[0] = pk_fma(splat(w[PAD + j]), tp, acc[0]);
                        acc[1] = pk_fma(splat(w[PAD + 1 + j]), tp, acc[1]);
                    });
                } else {
                    const float* w0 = buf + woff + pad;
                    static_for<HLEN>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        const v2f t = *reinterpret_cast<const v2f*>(w0 + j * fct);  // (even spacing: 8-byte aligned)
                        const v2f tp = f.t[HLEN - 1 - j];
                        acc[0] = pk_fma(splat(t.x), tp, acc[0]);
                        acc[1] = pk_fma(splat(t.y), tp, acc[1]);
                    });
                }
                ring[u][0] = acc[0];
                ring[u][1] = acc[1];
                // ---- column pass once the window r-HLEN+1 .. r is complete: output row m0 + r - (HLEN-1) of the class ----
                if (r >= HLEN - 1) {
                    v2f ah[2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}}, vd[2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}};  // (A, H) from lo, (V, D) from hi
                    static_for<HLEN>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        constexpr int s = (u + 1 + j) % HLEN;  // oldest row first
                        const v2f tp = f.t[HLEN - 1 - j];
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            ah[q] = pk_fma(splat(ring[s][q].x), tp, ah[q]);
                            vd[q] = pk_fma(splat(ring[s][q].y), tp, vd[q]);
                        }
                    });
                    if (wstore) {  // uniform; lanes without an output column are masked through EXEC, the instruction still counts
                        const size_t o = (size_t)(rho + fct * (m0 + r - (HLEN - 1))) * Nc;
                        asm_store_sm(cA + o, vox, v2f{ah[0].x, ah[1].x}, amask);
                        asm_store_sm_nt(cH + o, vox, v2f{ah[0].y, ah[1].y}, amask);
                        asm_store_sm_nt(cV + o, vox, v2f{vd[0].x, vd[1].x}, amask);
                        asm_store_sm_nt(cD + o, vox, v2f{vd[0].y, vd[1].y}, amask);
                    }
                }
            }
        });
    }
    asm_wait2<0>(pre0, pre1);  // (the clamped prefetch of the last step)
}
#endif

#if PDWT_SWTL2_PART >= 2
// inverse level: every staged row goes through the ROW synthesis first (u1 = IL_x(A) + IH_x(V), u2 = IL_x(H) + IH_x(D)), (u1, u2) enter
// the register ring and the COLUMN synthesis out = IL_y(u1) + IH_y(u2) emits one image row per input row (cf. k_swt_inv_fused4).
// One 8-byte LDS read per (band, tap): the column pair of the thread, already packed (any spacing: two dwords from a 4-byte-aligned
// address when the spacing is odd).
// FSEL = tap spacing known at compile time (1, 2, 4: LDS offsets become immediates), 0 = run-time spacing `fct`
template <int HLEN, int FSEL>
__global__ __launch_bounds__(256, 2) void k_swt_inv_fused2(const float* __restrict__ cA, const float* __restrict__ cH, const float* __restrict__ cV,
                                                            const float* __restrict__ cD, float* __restrict__ out, int Nr, int Nc, int fct, int M,
                                                            Taps2<float> f, int knob_xcd, const void* tbl)
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
    int bx, by;
    swt2_tile(knob_xcd, bx, by);
    const int rho = by % fct;
    const int m0 = (by / fct) * M;
    const int Mc = Nr / fct;
    const int nout = min(M, Mc - m0);
    if (nout <= 0) return;
    const int x0 = bx * kSwt2Tile;
    const int HLc = ((C * fct + 3) >> 2) << 2, HRc = (((HLEN - 1 - C) * fct + 3) >> 2) << 2;
    const int PW = HLc + kSwt2Tile + HRc;
    const int nst = PW >> 2;  // 16-byte chunks per staged row (<= 512)
    const int xs = x0 - HLc;
    const int xg = x0 + 2 * tid;
    const bool active = xg < Nc;
    const int nin = nout + HLEN - 1;
    const int k0 = min(tid, nst - 1), k1 = min(tid + 256, nst - 1);
    const int gc0 = wrapi(xs + 4 * k0, Nc), gc1 = wrapi(xs + 4 * k1, Nc);
    const int pad = HLc - C * fct;
    // The two banks live ONCE in SGPRs, as the aligned pairs (F[2m], F[2m+1]) the kernel arguments arrive in; row and column synthesis
    // both take tap F[HLEN-1-j] as one half of its pair (pk_fma_sbcast).  A splat per row tap plus reversed copies for the column taps
    // -- the form this kernel had first -- is 6 x HLEN scalar registers: the compiler spilled them to VGPR lanes and read every tap
    // back with v_readlane (2 per FMA: 6.7k / 12.8k / 15.6k of them in the 24 / 32 / 40-tap kernels).
    v2f npa[HLEN / 2], npb[HLEN / 2];
#pragma unroll
    for (int i = 0; i < HLEN / 2; i++) {
        npa[i] = v2f{f.a[2 * i], f.a[2 * i + 1]};
        npb[i] = v2f{f.b[2 * i], f.b[2 * i + 1]};
    }
    auto row_of = [&](int r) { return (size_t)(rho + fct * wrapi(m0 - C + min(r, nin - 1), Mc)) * Nc; };
    const float* const band[4] = {cA, cV, cH, cD};  // staging order: (A, V) feed u1, (H, D) feed u2
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
    v2f ru1[HLEN], ru2[HLEN];  // ring: (u1, u2) of the thread's 2 columns, packed

    for (int rb = 0; rb < nin; rb += HLEN) {
        static_for<HLEN>([&](auto U) {
            constexpr int u = decltype(U)::value;
            const int r = rb + u;
            if (r < nin) {
                float* const buf = smem + ((u & 1) ? 4 * PW : 0);
                wait_rows(wstore && r > HLEN - 1);  // (row r-1 stored its image row after these loads were issued)
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
                swt2_barrier();
                // ---- row synthesis: s[b] = sum_j band_b[x + (j - C) f] * tap_b[HLEN-1-j], the column pair packed ----
                v2f sacc[4];
                static_for<4>([&](auto B) {
                    constexpr int b = decltype(B)::value;
                    sacc[b] = v2f{0.f, 0.f};
                    int woff = b * PW + 2 * tid + pad;
                    asm("" : "+v"(woff) : "s"(r));  // (see swt_fused.inc: keeps the tap addresses out of loop-invariant registers)
                    const float* w0 = buf + woff;
                    // eight taps' column pairs are read before the first of them is used: counted waits, several reads in flight.  (The four
                    // bands in lockstep -- four independent accumulation chains instead of one at a time -- measured slower: db11 inverse
                    // levels 805 -> 937 us, db16 1146 -> 1165: the kernel is bound by its LDS traffic, not by the FMA chains.)
                    constexpr int G = 8;
                    static_for<HLEN / G>([&](auto GG) {
                        constexpr int g = decltype(GG)::value;
                        v2f t[G];
                        static_for<G>([&](auto Q) {
                            constexpr int q = decltype(Q)::value;
                            const float* p = w0 + (g * G + q) * (FSEL ? FSEL : fct);
                            t[q] = v2f{p[0], p[1]};
                        });
                        static_for<G>([&](auto Q) {
                            constexpr int q = decltype(Q)::value;
                            constexpr int idx = HLEN - 1 - (g * G + q);  // tap F[idx] = half (idx & 1) of pair idx >> 1
                            if constexpr (b & 1) sacc[b] = pk_fma_sbcast<idx & 1, false>(t[q], npb[idx >> 1], sacc[b]);
                            else sacc[b] = pk_fma_sbcast<idx & 1, false>(t[q], npa[idx >> 1], sacc[b]);
                        });
                    });
                });
                ru1[u] = sacc[0] + sacc[1];  // band[]: 0 = A (IL), 1 = V (IH), 2 = H (IL), 3 = D (IH)
                ru2[u] = sacc[2] + sacc[3];
                // ---- column synthesis: out = IL_y(u1) + IH_y(u2) over the window r-HLEN+1 .. r ----
                if (r >= HLEN - 1) {
                    v2f o1 = {0.f, 0.f}, o2 = {0.f, 0.f};
                    static_for<HLEN>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        constexpr int s = (u + 1 + j) % HLEN;
                        constexpr int idx = HLEN - 1 - j;
                        o1 = pk_fma_sbcast<idx & 1, false>(ru1[s], npa[idx >> 1], o1);
                        o2 = pk_fma_sbcast<idx & 1, false>(ru2[s], npb[idx >> 1], o2);
                    });
                    if (wstore) asm_store_sm(out + (size_t)(rho + fct * (m0 + r - (HLEN - 1))) * Nc, vox, o1 + o2, amask);
                }
            }
        });
    }
    wait_rows(false);  // (the clamped prefetch of the last step)
}
#endif

#define PDWT_CHECK_LAUNCH() PDWT_HIP_TRY(hipGetLastError())
#ifndef PDWT_SWTL2_HLENS  // (experiment builds restrict the list)
#define PDWT_SWTL2_HLENS(X) X(24) X(32) X(40)
#endif

// the bank of hlen taps inside the next instantiated length: q zero taps at either end
static inline int swt2_padded_len(int hlen) { return hlen <= 24 ? 24 : (hlen <= 32 ? 32 : 40); }
static inline Taps2<float> swt2_pad(const Taps2<float>& f, int hlen, int H)
{
    Taps2<float> p;
    const int q = (H - hlen) / 2;
    for (int k = 0; k < PDWT_MAX_FILTER_WIDTH; k++) {
        const bool in = k >= q && k < q + hlen;
        p.a[k] = in ? f.a[k - q] : 0.f;
        p.b[k] = in ? f.b[k - q] : 0.f;
    }
    return p;
}
// rows of a class per workgroup: as many workgroups as are resident at once (two per CU at these register counts), at least the ring
static inline int swt2_rows(int Mc, int fct, int tiles, int H, int knob_m, int nimg)
{
    int M = knob_m;
    if (M <= 0) {
        M = (int)(((long long)Mc * fct * tiles * nimg + 511) / 512);
        if (M < H) M = H;
    }
    return M > Mc ? Mc : M;
}

#if PDWT_SWTL2_PART == 1
template <int HLEN>
static int launch_swt_fwd2(const float* in, float* cA, float* cH, float* cV, float* cD, int Nr, int Nc, int fct, const Taps2<float>& f2, const void* d_tbl,
                           int nimg)
{
    constexpr int C = HLEN / 2 - 1;
    TapsLH f;
    for (int k = 0; k < PDWT_MAX_FILTER_WIDTH; k++) f.t[k] = v2f{f2.a[k], f2.b[k]};
    const int HLc = ((C * fct + 3) >> 2) << 2, HRc = (((HLEN - 1 - C) * fct + 3) >> 2) << 2;
    const int PW = HLc + kSwt2Tile + HRc;
    if (PW / 4 > 512 || PW - kSwt2Tile > Nc) return 1;  // two staging chunks per thread; halo shorter than a row
    const size_t lds = 2 * (size_t)PW * sizeof(float) + 64;
    const int Mc = Nr / fct, tiles = idiv_up(Nc, kSwt2Tile);
    const int M = swt2_rows(Mc, fct, tiles, HLEN, knob(KN_SWTF_M), nimg);
    dim3 grid(tiles, fct * idiv_up(Mc, M), nimg);
    stat_hit(ST_SWTL2_FWD);
    KTimer kt(K_SWT_ANA_COLS, true);
    if (fct == 1) PDWT_LAUNCH_KT(kt, (k_swt_fwd_fused2<HLEN, true>), grid, dim3(256), lds, in, cA, cH, cV, cD, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), d_tbl);
    else PDWT_LAUNCH_KT(kt, (k_swt_fwd_fused2<HLEN, false>), grid, dim3(256), lds, in, cA, cH, cV, cD, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), d_tbl);
    PDWT_CHECK_LAUNCH();
    return PDWT_OK;
}
// (geometry and aliasing already checked by swt_fwd_fused_f32)
int swt_fwd_fused_l2_f32(const float* in, float* cA, float* cH, float* cV, float* cD, int Nr, int Nc, int hlen, int fct, const Taps2<float>& f,
                         const void* d_tbl, int nimg)
{
    if (knob(KN_SWTF_LONG) != 1 || hlen < 22 || hlen > 40 || (hlen & 1) || (Nc & 3)) return 1;
    const int H = swt2_padded_len(hlen);
    if (Nr / fct < 2 * H) return 1;
    const Taps2<float> p = swt2_pad(f, hlen, H);
    switch (H) {
#define X(HH) \
    case HH: return launch_swt_fwd2<HH>(in, cA, cH, cV, cD, Nr, Nc, fct, p, d_tbl, nimg);
        PDWT_SWTL2_HLENS(X)
#undef X
        default: return 1;
    }
}
#endif

#if PDWT_SWTL2_PART >= 2
#define PDWT_SWT2_INV_ARGS                                                                                                        \
    int H, KTimer &kt, dim3 grid, size_t lds, const float *cA, const float *cH, const float *cV, const float *cD, float *out, int Nr, \
        int Nc, int fct, int M, const Taps2<float>&f, int knob_xcd, const void *d_tbl
// the kernels with a compile-time tap spacing (LDS offsets as immediates: inverse levels of db16 at 4096^2 1150 -> 987 us for three
// levels) live in translation units of their own -- swt_fused_l2_inv1 / _inv2 / _inv4.hip, ~5 minutes of compile time each
int swt2_inv_fsel1(PDWT_SWT2_INV_ARGS);
int swt2_inv_fsel2(PDWT_SWT2_INV_ARGS);
int swt2_inv_fsel4(PDWT_SWT2_INV_ARGS);
#endif
#if PDWT_SWTL2_PART == 3
#define SWT2_CAT_(a, b) a##b
#define SWT2_CAT(a, b) SWT2_CAT_(a, b)
int SWT2_CAT(swt2_inv_fsel, PDWT_SWTL2_FSEL)(PDWT_SWT2_INV_ARGS)
{
    switch (H) {
#define X(HH)                                                                                                                              \
    case HH:                                                                                                                               \
        PDWT_LAUNCH_KT(kt, (k_swt_inv_fused2<HH, PDWT_SWTL2_FSEL>), grid, dim3(256), lds, cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob_xcd, d_tbl); \
        break;
        PDWT_SWTL2_HLENS(X)
#undef X
        default: return 1;
    }
    PDWT_CHECK_LAUNCH();
    return PDWT_OK;
}
#endif

#if PDWT_SWTL2_PART == 2
template <int HLEN>
static int launch_swt_inv2(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int fct,
                           const Taps2<float>& f, const void* d_tbl, int nimg)
{
    constexpr int C = HLEN / 2;
    const int HLc = ((C * fct + 3) >> 2) << 2, HRc = (((HLEN - 1 - C) * fct + 3) >> 2) << 2;
    const int PW = HLc + kSwt2Tile + HRc;
    if (PW / 4 > 512 || PW - kSwt2Tile > Nc) return 1;
    const size_t lds = 2 * 4 * (size_t)PW * sizeof(float) + 64;
    if (lds > 64 * 1024) return 1;
    const int Mc = Nr / fct, tiles = idiv_up(Nc, kSwt2Tile);
    const int M = swt2_rows(Mc, fct, tiles, HLEN, knob(KN_SWTF_MI), nimg);
    dim3 grid(tiles, fct * idiv_up(Mc, M), nimg);
    stat_hit(ST_SWTL2_INV);
    KTimer kt(K_SWT_SYN_COLS, true);
    if (fct == 1) return swt2_inv_fsel1(HLEN, kt, grid, lds, cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), d_tbl);
    if (fct == 2) return swt2_inv_fsel2(HLEN, kt, grid, lds, cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), d_tbl);
    if (fct == 4) return swt2_inv_fsel4(HLEN, kt, grid, lds, cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), d_tbl);
    PDWT_LAUNCH_KT(kt, (k_swt_inv_fused2<HLEN, 0>), grid, dim3(256), lds, cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD), d_tbl);
    PDWT_CHECK_LAUNCH();
    return PDWT_OK;
}
int swt_inv_fused_l2_f32(const float* cA, const float* cH, const float* cV, const float* cD, float* out, int Nr, int Nc, int hlen, int fct,
                         const Taps2<float>& f, const void* d_tbl, int nimg)
{
    if (knob(KN_SWTF_LONG) != 1 || hlen < 22 || hlen > 40 || (hlen & 1) || (Nc & 3)) return 1;
    const int H = swt2_padded_len(hlen);
    if (Nr / fct < 2 * H) return 1;
    const Taps2<float> p = swt2_pad(f, hlen, H);
    switch (H) {
#define X(HH) \
    case HH: return launch_swt_inv2<HH>(cA, cH, cV, cD, out, Nr, Nc, fct, p, d_tbl, nimg);
        PDWT_SWTL2_HLENS(X)
#undef X
        default: return 1;
    }
}
#endif

}  // namespace pdwt
