// swt_fused_f64.inc -- one level of the 2-D stationary transform per launch, DOUBLE precision: the structure of swt_fused.inc
// (rows of a residue class streamed through LDS, row pass out of LDS, column pass on a register ring) with two columns per thread
// (one 16-byte access) and a 512-column tile.  Same sums in the same order as the two-pass kernels (forward: bit-identical; the
// inverse runs rows before columns like its float32 counterpart: equal within a few ulp).
// Reference code replaced: w_kern_forward_swt_pass1/2, w_kern_inverse_swt_pass1/2 and one iteration of their level loops
// (src/separable.cu:409-537, 553-672).  PDWT_SWTD_PART: 1 = forward, 2 = inverse (separate translation units).
#include "swt_fused.hpp"

#include "stream_dev.hpp"

namespace pdwt {

namespace {
constexpr int kSwtTileD = 512;  // columns per workgroup: 256 threads x 2
typedef double v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void swtd_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// XCD-aware tile order (see swt_fused.inc)
__device__ __forceinline__ void swtd_tile(int knob_xcd, int& bx, int& by)
{
    const int T = gridDim.x * gridDim.y, w = blockIdx.y * gridDim.x + blockIdx.x;
    const int xq = w & 7, per = T >> 3, rem = T & 7;
    const int Lw = knob_xcd ? xq * per + min(xq, rem) + (w >> 3) : w;
    bx = Lw % (int)gridDim.x;
    by = Lw / (int)gridDim.x;
}
__host__ __device__ constexpr int up2(int v) { return (v + 1) & ~1; }
}  // namespace

#if PDWT_SWTD_PART == 1
// FSEL: 1 = tap spacing 1 (the row-pass window is one run of aligned 16-byte chunks), 0 = even spacing (every tap its own aligned read)
template <int HLEN, int FSEL>
__global__ __launch_bounds__(256) void k_swt_fwd_fused_d(const double* __restrict__ in, double* __restrict__ cA, double* __restrict__ cH,
                                                          double* __restrict__ cV, double* __restrict__ cD, int Nr, int Nc, int fct, int M,
                                                          Taps2<double> f, int knob_xcd)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* const smem = reinterpret_cast<double*>(smem_raw);
    constexpr int C = HLEN / 2 - 1;
    const int tid = threadIdx.x;
    int bx, by;
    swtd_tile(knob_xcd, bx, by);
    const int rho = by % fct;
    const int m0 = (by / fct) * M;
    const int Mc = Nr / fct;  // rows of one residue class
    const int nout = min(M, Mc - m0);
    if (nout <= 0) return;
    const int x0 = bx * kSwtTileD;
    const int HLc = up2(C * fct), HRc = up2((HLEN - 1 - C) * fct);
    const int PW = HLc + kSwtTileD + HRc;  // staged doubles per row
    const int nst = PW >> 1;               // 16-byte chunks per staged row (<= 512: checked by the dispatcher)
    const int xs = x0 - HLc;               // global column of LDS index 0 (even, may be negative)
    const int xg = x0 + 2 * tid;
    const bool active = xg < Nc;
    const int nin = nout + HLEN - 1;
    const int k0 = min(tid, nst - 1), k1 = min(tid + 256, nst - 1);
    const int gc0 = wrapi(xs + 2 * k0, Nc), gc1 = wrapi(xs + 2 * k1, Nc);  // (Nc is even: a chunk never straddles the wrap)
    auto row_of = [&](int r) { return (size_t)(rho + fct * wrapi(m0 - C + min(r, nin - 1), Mc)) * Nc; };
    v2d pre0, pre1;
    {
        const double* p = in + row_of(0);
        pre0 = *reinterpret_cast<const v2d*>(p + gc0);
        pre1 = *reinterpret_cast<const v2d*>(p + gc1);
    }
    double rlo[HLEN][2], rhi[HLEN][2];  // row-pass results of the thread's 2 columns for the last HLEN rows of the class

    for (int rb = 0; rb < nin; rb += HLEN) {
        static_for<HLEN>([&](auto U) __attribute__((always_inline)) {
            constexpr int u = decltype(U)::value;
            const int r = rb + u;
            if (r < nin) {  // uniform
                double* const buf = smem + ((u & 1) ? PW : 0);
                reinterpret_cast<v2d*>(buf)[k0] = pre0;
                reinterpret_cast<v2d*>(buf)[k1] = pre1;
                {
                    const double* p = in + row_of(r + 1);
                    pre0 = *reinterpret_cast<const v2d*>(p + gc0);
                    pre1 = *reinterpret_cast<const v2d*>(p + gc1);
                }
                swtd_barrier();
                // ---- row pass: (lo,hi)[q] = sum_j x[2 tid + q + (j - C) f] * (L,H)[HLEN-1-j] ----
                double lo[2] = {0.0, 0.0}, hi[2] = {0.0, 0.0};
                if constexpr (FSEL == 0) {
                    int woff = 2 * tid;  // HLc == C*f here (even spacing); laundered per row (see swt_fused.inc)
                    asm("" : "+v"(woff) : "s"(r));
                    const double* w0 = buf + woff;
                    static_for<HLEN>([&](auto J) __attribute__((always_inline)) {
                        constexpr int j = decltype(J)::value;
                        const v2d t = *reinterpret_cast<const v2d*>(w0 + j * fct);
                        const double tl = f.a[HLEN - 1 - j], th = f.b[HLEN - 1 - j];
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            lo[q] = __builtin_fma(t[q], tl, lo[q]);
                            hi[q] = __builtin_fma(t[q], th, hi[q]);
                        }
                    });
                } else {
                    constexpr int PAD = up2(C) - C;                      // window start inside its first chunk
                    constexpr int NCH = (PAD + 2 + (HLEN - 1) + 1) / 2;  // aligned chunks covering the window
                    double w[NCH * 2];
#pragma unroll
                    for (int k = 0; k < NCH; k++) {
                        const v2d t = reinterpret_cast<const v2d*>(buf + 2 * tid)[k];
                        w[2 * k] = t[0];
                        w[2 * k + 1] = t[1];
                    }
                    static_for<HLEN>([&](auto J) __attribute__((always_inline)) {
                        constexpr int j = decltype(J)::value;
                        const double tl = f.a[HLEN - 1 - j], th = f.b[HLEN - 1 - j];
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            lo[q] = __builtin_fma(w[PAD + q + j], tl, lo[q]);
                            hi[q] = __builtin_fma(w[PAD + q + j], th, hi[q]);
                        }
                    });
                }
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    rlo[u][q] = lo[q];
                    rhi[u][q] = hi[q];
                }
                // ---- column pass once the window r-HLEN+1 .. r is complete: output row m0 + r - (HLEN-1) of the class ----
                if (r >= HLEN - 1) {
                    double a[2] = {0.0, 0.0}, h[2] = {0.0, 0.0}, v[2] = {0.0, 0.0}, d[2] = {0.0, 0.0};
                    static_for<HLEN>([&](auto J) __attribute__((always_inline)) {
                        constexpr int j = decltype(J)::value;
                        constexpr int s = (u + 1 + j) % HLEN;  // oldest row first
                        const double tl = f.a[HLEN - 1 - j], th = f.b[HLEN - 1 - j];
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            a[q] = __builtin_fma(rlo[s][q], tl, a[q]);
                            h[q] = __builtin_fma(rlo[s][q], th, h[q]);
                            v[q] = __builtin_fma(rhi[s][q], tl, v[q]);
                            d[q] = __builtin_fma(rhi[s][q], th, d[q]);
                        }
                    });
                    if (active) {
                        const size_t o = (size_t)(rho + fct * (m0 + r - (HLEN - 1))) * Nc + xg;
                        *reinterpret_cast<v2d*>(cA + o) = v2d{a[0], a[1]};
                        *reinterpret_cast<v2d*>(cH + o) = v2d{h[0], h[1]};
                        *reinterpret_cast<v2d*>(cV + o) = v2d{v[0], v[1]};
                        *reinterpret_cast<v2d*>(cD + o) = v2d{d[0], d[1]};
                    }
                }
            }
        });
    }
}
#else
// inverse level: every staged row goes through the ROW synthesis first, u1 = IL_x(A) + IH_x(V), u2 = IL_x(H) + IH_x(D); (u1, u2) enter the
// register ring and the COLUMN synthesis out = IL_y(u1) + IH_y(u2) emits one image row per input row (see swt_fused.inc)
template <int HLEN, int FSEL>
__global__ __launch_bounds__(256) void k_swt_inv_fused_d(const double* __restrict__ cA, const double* __restrict__ cH, const double* __restrict__ cV,
                                                          const double* __restrict__ cD, double* __restrict__ out, int Nr, int Nc, int fct, int M,
                                                          Taps2<double> f, int knob_xcd)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* const smem = reinterpret_cast<double*>(smem_raw);
    constexpr int C = HLEN / 2;  // synthesis centre (A-4)
    const int tid = threadIdx.x;
    int bx, by;
    swtd_tile(knob_xcd, bx, by);
    const int rho = by % fct;
    const int m0 = (by / fct) * M;
    const int Mc = Nr / fct;
    const int nout = min(M, Mc - m0);
    if (nout <= 0) return;
    const int x0 = bx * kSwtTileD;
    const int HLc = up2(C * fct), HRc = up2((HLEN - 1 - C) * fct);
    const int PW = HLc + kSwtTileD + HRc;
    const int nst = PW >> 1;
    const int xs = x0 - HLc;
    const int xg = x0 + 2 * tid;
    const bool active = xg < Nc;
    const int nin = nout + HLEN - 1;
    const int k0 = min(tid, nst - 1), k1 = min(tid + 256, nst - 1);
    const int gc0 = wrapi(xs + 2 * k0, Nc), gc1 = wrapi(xs + 2 * k1, Nc);
    auto row_of = [&](int r) { return (size_t)(rho + fct * wrapi(m0 - C + min(r, nin - 1), Mc)) * Nc; };
    const double* const band[4] = {cA, cV, cH, cD};  // staging order: (A,V) feed u1, (H,D) feed u2
    v2d pre[4][2];
    {
        const size_t o = row_of(0);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            pre[b][0] = *reinterpret_cast<const v2d*>(band[b] + o + gc0);
            pre[b][1] = *reinterpret_cast<const v2d*>(band[b] + o + gc1);
        }
    }
    double ru1[HLEN][2], ru2[HLEN][2];  // ring: (u1, u2) of the thread's 2 columns

    for (int rb = 0; rb < nin; rb += HLEN) {
        static_for<HLEN>([&](auto U) __attribute__((always_inline)) {
            constexpr int u = decltype(U)::value;
            const int r = rb + u;
            if (r < nin) {
                double* const buf = smem + ((u & 1) ? 4 * PW : 0);
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    reinterpret_cast<v2d*>(buf + b * PW)[k0] = pre[b][0];
                    reinterpret_cast<v2d*>(buf + b * PW)[k1] = pre[b][1];
                }
                {
                    const size_t o = row_of(r + 1);
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        pre[b][0] = *reinterpret_cast<const v2d*>(band[b] + o + gc0);
                        pre[b][1] = *reinterpret_cast<const v2d*>(band[b] + o + gc1);
                    }
                }
                swtd_barrier();
                // ---- row synthesis: s[b] = sum_j band_b[x + (j - C) f] * tap_b[HLEN-1-j] ----
                double sacc[4][2];
                static_for<4>([&](auto B) __attribute__((always_inline)) {
                    constexpr int b = decltype(B)::value;
                    sacc[b][0] = sacc[b][1] = 0.0;
                    int woff = b * PW + 2 * tid;
                    asm("" : "+v"(woff) : "s"(r));
                    const double* w0 = buf + woff;
                    if constexpr (FSEL == 0) {
                        static_for<HLEN>([&](auto J) __attribute__((always_inline)) {
                            constexpr int j = decltype(J)::value;
                            const v2d t = *reinterpret_cast<const v2d*>(w0 + j * fct);
                            const double tp = (b & 1) ? f.b[HLEN - 1 - j] : f.a[HLEN - 1 - j];
                            sacc[b][0] = __builtin_fma(t[0], tp, sacc[b][0]);
                            sacc[b][1] = __builtin_fma(t[1], tp, sacc[b][1]);
                        });
                    } else {
                        constexpr int PAD = up2(C) - C;
                        constexpr int NCH = (PAD + 2 + (HLEN - 1) + 1) / 2;
                        double w[NCH * 2];
#pragma unroll
                        for (int k = 0; k < NCH; k++) {
                            const v2d t = reinterpret_cast<const v2d*>(w0)[k];
                            w[2 * k] = t[0];
                            w[2 * k + 1] = t[1];
                        }
                        static_for<HLEN>([&](auto J) __attribute__((always_inline)) {
                            constexpr int j = decltype(J)::value;
                            const double tp = (b & 1) ? f.b[HLEN - 1 - j] : f.a[HLEN - 1 - j];
                            sacc[b][0] = __builtin_fma(w[PAD + j], tp, sacc[b][0]);
                            sacc[b][1] = __builtin_fma(w[PAD + 1 + j], tp, sacc[b][1]);
                        });
                    }
                });
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    ru1[u][q] = sacc[0][q] + sacc[1][q];  // band[]: 0 = A (IL), 1 = V (IH), 2 = H (IL), 3 = D (IH)
                    ru2[u][q] = sacc[2][q] + sacc[3][q];
                }
                // ---- column synthesis: out = IL_y(u1) + IH_y(u2) over the window r-HLEN+1 .. r ----
                if (r >= HLEN - 1) {
                    double o1[2] = {0.0, 0.0}, o2[2] = {0.0, 0.0};
                    static_for<HLEN>([&](auto J) __attribute__((always_inline)) {
                        constexpr int j = decltype(J)::value;
                        constexpr int s = (u + 1 + j) % HLEN;
                        const double ta = f.a[HLEN - 1 - j], tb = f.b[HLEN - 1 - j];
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            o1[q] = __builtin_fma(ru1[s][q], ta, o1[q]);
                            o2[q] = __builtin_fma(ru2[s][q], tb, o2[q]);
                        }
                    });
                    if (active) *reinterpret_cast<v2d*>(out + (size_t)(rho + fct * (m0 + r - (HLEN - 1))) * Nc + xg) = v2d{o1[0] + o2[0], o1[1] + o2[1]};
                }
            }
        });
    }
}
#endif

#define PDWT_CHECK_LAUNCH() PDWT_HIP_TRY(hipGetLastError())
#define PDWT_SWTD_HLENS(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16)

// rows of a class per workgroup (the float32 kernels' measured optimum scaled to this tile: ~512-700 workgroups)
static int swtd_chunk_rows(int Mc, int fct, int tiles, int hlen, int wgs, int forced)
{
    int M = forced;
    if (M <= 0) {
        M = (int)(((long long)Mc * fct * tiles + wgs - 1) / wgs);
        if (M < hlen) M = hlen;
    }
    return M > Mc ? Mc : M;
}

#if PDWT_SWTD_PART == 1
template <int HLEN>
static int launch_swt_fwd_d(const double* in, double* cA, double* cH, double* cV, double* cD, int Nr, int Nc, int fct, const Taps2<double>& f)
{
    constexpr int C = HLEN / 2 - 1;
    const int PW = up2(C * fct) + kSwtTileD + up2((HLEN - 1 - C) * fct);
    if (PW / 2 > 512 || PW - kSwtTileD > Nc) return 1;  // two staging chunks per thread; halo shorter than a row
    const size_t lds = 2 * (size_t)PW * sizeof(double) + 64;
    const int Mc = Nr / fct, tiles = idiv_up(Nc, kSwtTileD);
    const int M = swtd_chunk_rows(Mc, fct, tiles, HLEN, 704, knob(KN_SWTF_M));
    dim3 grid(tiles, fct * idiv_up(Mc, M));
    stat_hit(ST_SWTD_FWD);
    KTimer kt(K_SWT_ANA_COLS);
    if (fct == 1) hipLaunchKernelGGL((k_swt_fwd_fused_d<HLEN, 1>), grid, dim3(256), lds, stream(), in, cA, cH, cV, cD, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD));
    else hipLaunchKernelGGL((k_swt_fwd_fused_d<HLEN, 0>), grid, dim3(256), lds, stream(), in, cA, cH, cV, cD, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD));
    PDWT_CHECK_LAUNCH();
    return PDWT_OK;
}

int swt_fwd_fused_f64(const double* in, double* cA, double* cH, double* cV, double* cD, int Nr, int Nc, int hlen, int fct, const Taps2<double>& f)
{
    if (knob(KN_SWTF) != 1 || knob(KN_SWTF_F64) != 1) return 1;
    if ((Nc & 1) || Nc < 64 || (Nr % fct) != 0 || Nr / fct < 2 * hlen) return 1;
    if (!al16(in) || !al16(cA) || !al16(cH) || !al16(cV) || !al16(cD)) return 1;
    if (in == cA || in == cH || in == cV || in == cD) return 1;  // one launch: the input must not be a band being written
    switch (hlen) {
#define X(H) \
    case H: return launch_swt_fwd_d<H>(in, cA, cH, cV, cD, Nr, Nc, fct, f);
        PDWT_SWTD_HLENS(X)
#undef X
        default: return 1;
    }
}
#else
template <int HLEN>
static int launch_swt_inv_d(const double* cA, const double* cH, const double* cV, const double* cD, double* out, int Nr, int Nc, int fct,
                            const Taps2<double>& f)
{
    constexpr int C = HLEN / 2;
    const int PW = up2(C * fct) + kSwtTileD + up2((HLEN - 1 - C) * fct);
    if (PW / 2 > 512 || PW - kSwtTileD > Nc) return 1;
    const size_t lds = 2 * 4 * (size_t)PW * sizeof(double) + 64;
    if (lds > 64 * 1024) return 1;
    const int Mc = Nr / fct, tiles = idiv_up(Nc, kSwtTileD);
    const int M = swtd_chunk_rows(Mc, fct, tiles, HLEN, 512, knob(KN_SWTF_MI));
    dim3 grid(tiles, fct * idiv_up(Mc, M));
    stat_hit(ST_SWTD_INV);
    KTimer kt(K_SWT_SYN_COLS);
    if (fct == 1) hipLaunchKernelGGL((k_swt_inv_fused_d<HLEN, 1>), grid, dim3(256), lds, stream(), cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD));
    else hipLaunchKernelGGL((k_swt_inv_fused_d<HLEN, 0>), grid, dim3(256), lds, stream(), cA, cH, cV, cD, out, Nr, Nc, fct, M, f, knob(KN_SWTF_XCD));
    PDWT_CHECK_LAUNCH();
    return PDWT_OK;
}

int swt_inv_fused_f64(const double* cA, const double* cH, const double* cV, const double* cD, double* out, int Nr, int Nc, int hlen, int fct,
                      const Taps2<double>& f)
{
    if (knob(KN_SWTF) != 1 || knob(KN_SWTF_F64) != 1) return 1;
    if ((Nc & 1) || Nc < 64 || (Nr % fct) != 0 || Nr / fct < 2 * hlen) return 1;
    if (!al16(out) || !al16(cA) || !al16(cH) || !al16(cV) || !al16(cD)) return 1;
    if (out == cA || out == cH || out == cV || out == cD) return 1;
    switch (hlen) {
#define X(H) \
    case H: return launch_swt_inv_d<H>(cA, cH, cV, cD, out, Nr, Nc, fct, f);
        PDWT_SWTD_HLENS(X)
#undef X
        default: return 1;
    }
}
#endif

}  // namespace pdwt
