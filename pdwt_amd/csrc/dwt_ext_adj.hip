// dwt_ext_adj.hip -- the adjoint operators of the transforms with signal-extension boundary modes (include/pdwt_hip.h "Adjoints of the
// boundary-mode DWT"): what a gradient method needs of pdwt_ext2db_* and pdwt_ext1d_*.  The stages are the functions of
// dwt_ext_adj.hpp; the mathematics is stated there.
//   adjoint of the forward (a mode): per level, coarse to fine, a synthesis with the REVERSED ANALYSIS taps onto the extended grid,
//   then the fold of the extension.
//     k_ext_adj_syn        2-D, 32 x 64 cells of the extended grid of image blockIdx.z per workgroup (the tile of k_ext3_inv_xy): stage
//                          the four padded cotangent windows, column synthesis into LDS, row synthesis; a cell of the sample range goes
//                          straight to the output, a cell of the halo to the packed frame in scratch
//     k_ext_adj_fold       2-D, 32 x 8 samples per workgroup: a tile inside the interior run of both axes (computed on the host from
//                          ext_index) leaves at once; else the index maps of the halo cells of both axes go to LDS and a workgroup whose
//                          tile no halo cell maps into leaves; a sample with pre-images adds them (its own cell plus frame cells)
//                          in ascending (sy, sx) and is rewritten.  No atomics: the result does not depend on B or on the tiling.
//     k_ext1d_adj / k_ext1d_adj_fold   the same along the rows of a batch, (tile, row) flattened on grid.x
//     k_ext1d_adj_fused    ALL levels of a pack of rows in one launch, the pipeline of k_ext1d_inv_fused with the fold as one more
//                          stage: the synthesis of a level writes the extended line (the halo cells the forward reserves), barrier,
//                          fold, barrier; the folded line, its padding zeroed, is the approximation cotangent of the next level
//   adjoint of the inverse (no mode): exactly the forward transform in mode zero with the bank L' = reversed IL, H' = reversed IH; no
//   kernel of its own, the driver builds the bank and runs pdwt_ext2db_forward_* / pdwt_ext1d_forward_* (fused forms included).
// Traffic of a 2-D level per image: the four cotangent bands read once (plus tile halos), nr nc + frame written once, and the fold reads
// and rewrites only samples with pre-images (at most 2 F rows and columns) plus their frame cells.
#include <algorithm>

#include "dwt_ext_adj.hpp"
#include "dwt_ext3d_xy.hpp"

namespace pdwt {

constexpr int kAdjThreads = 256;  // the fold kernel (the synthesis kernel: kTileThreads)
constexpr int AFY = 32, AFX = 8;  // fold tile (samples)
constexpr int kAdjMaxBatch = 65535;
constexpr int kAdjMaxLev = 32;

template <typename T>
struct AdjJob {
    T* dst;          // (B, nr, nc)
    const T* q[4];   // cotangents of A, H, V, D: (B, hr, hc) each
    T* frame;        // (B, frame_elems), NULL in mode zero
    int nr, nc, hr, hc, mode;
};

template <typename T, int HL>
__global__ __launch_bounds__(kTileThreads) void k_ext_adj_syn(AdjJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];
    constexpr int WR = tile_inv_win(TIY, HL, false), WC = tile_inv_win(TIX, HL, false);
    T* in = reinterpret_cast<T*>(smem_d);  // [4][WR][WC]
    T* cb = in + 4 * WR * WC;              // [2][TIY][WC]
    const int tid = threadIdx.x;
    const int g0x = blockIdx.x * TIX, g0y = blockIdx.y * TIY;  // even cells of the extended grid
    const int Er = adj_ext_len(job.nr, HL), Ec = adj_ext_len(job.nc, HL);
    const size_t zoff = (size_t)blockIdx.z * job.hr * job.hc;
    const T* const q[4] = {job.q[0] + zoff, job.q[1] + zoff, job.q[2] + zoff, job.q[3] + zoff};
    // the windows of the PADDED bands: the origin in band coordinates may be negative
    ext_stage_children<T, WR, WC, kTileThreads>(in, q, job.hr, job.hc, g0y / 2 - (HL / 2 - 1), g0x / 2 - (HL / 2 - 1), tid);
    tile_cols_synthesis<T, HL, 0, WR, WC, TIY, kTileThreads>(in, cb, taps, tid);
    T* frame = job.frame ? job.frame + (size_t)blockIdx.z * adj_frame_elems(job.nr, job.nc, HL) : nullptr;
    adj_rows_synthesis_write<T, HL, WC, TIY, TIX, kTileThreads>(cb, taps, job.dst + (size_t)blockIdx.z * job.nr * job.nc, frame, job.nr, job.nc, Er, Ec, g0y,
                                                                g0x, tid);
}

// the longest run of samples [y0, y1) x [x0, x1) of either axis that no halo cell repeats (host; from ext_index): a tile inside both runs
// has nothing to fold and leaves before it computes anything
struct AdjGap {
    int y0, y1, x0, x1;
};
static void adj_gap(int n, int F, int mode, int& g0, int& g1)
{
    int t[2 * PDWT_MAX_FILTER_WIDTH], cnt = 0;
    for (int h = 0; h < adj_halo_len(n, F); h++)
        if (const int k = ext_index(adj_halo_s(h, n, F), n, mode); k >= 0) t[cnt++] = k;
    std::sort(t, t + cnt);
    g0 = 0, g1 = cnt ? t[0] : n;
    for (int i = 0; i < cnt; i++) {
        const int a = t[i] + 1, b = i + 1 < cnt ? t[i + 1] : n;
        if (b - a > g1 - g0) g0 = a, g1 = b;
    }
}

template <typename T>
__global__ __launch_bounds__(kAdjThreads) void k_ext_adj_fold(T* __restrict__ dst, const T* __restrict__ frame, int nr, int nc, int F, int mode, AdjGap gap)
{
    __shared__ int maps[4 * PDWT_MAX_FILTER_WIDTH];  // rmap[Hr] | cmap[Hc], each at most 2 F - 3
    const int tid = threadIdx.x;
    const int Hr = adj_halo_len(nr, F), Hc = adj_halo_len(nc, F);
    const int y0 = blockIdx.y * AFY, x0 = blockIdx.x * AFX;
    if (y0 >= gap.y0 && y0 + AFY <= gap.y1 && x0 >= gap.x0 && x0 + AFX <= gap.x1) return;  // (uniform) the interior of the image
    int hit = 0;
    for (int h = tid; h < Hr + Hc; h += kAdjThreads) {
        const bool row = h < Hr;
        const int m = row ? ext_index(adj_halo_s(h, nr, F), nr, mode) : ext_index(adj_halo_s(h - Hr, nc, F), nc, mode);
        maps[h] = m;
        hit |= row ? (m >= y0 && m < y0 + AFY) : (m >= x0 && m < x0 + AFX);
    }
    if (!__syncthreads_or(hit)) return;  // no halo cell repeats a sample of this tile
    const int y = y0 + tid / AFX, x = x0 + tid % AFX;
    if (y >= nr || x >= nc) return;
    adj_fold_sample<T>(dst + (size_t)blockIdx.z * nr * nc, frame + (size_t)blockIdx.z * adj_frame_elems(nr, nc, F), maps, maps + Hr, y, x, nr, nc, F);
}

// ---- 1-D ------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kExt1dThreads) void k_ext1d_adj(T* __restrict__ dst, const T* __restrict__ a, const T* __restrict__ d, T* __restrict__ halo, int n, int N,
                                                            int tiles, int hlen, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int WMAX = kExt1dTile + PDWT_MAX_FILTER_WIDTH / 2;
    T* wa = reinterpret_cast<T*>(smem);  // [kExt1dTile + hlen / 2 - 1]
    T* wd = wa + WMAX;
    const int tid = threadIdx.x;
    const unsigned row = blockIdx.x / (unsigned)tiles, tile = blockIdx.x - row * (unsigned)tiles;
    const int P = N + hlen / 2 - 1, p0 = (int)tile * kExt1dTile, cntp = P - p0 < kExt1dTile ? P - p0 : kExt1dTile;
    const int w = cntp + hlen / 2 - 1;
    ext1d_adj_stage<T, kExt1dThreads>(wa, a + (size_t)row * N, N, hlen, p0, w, tid);
    ext1d_adj_stage<T, kExt1dThreads>(wd, d + (size_t)row * N, N, hlen, p0, w, tid);
    lds_barrier();
    ext1d_adj_tile<T, kExt1dThreads>(wa, wd, p0, cntp, n, hlen, taps, dst + (size_t)row * n, halo ? halo + (size_t)row * adj_halo_len(n, hlen) : nullptr, tid);
}

// RB rows per workgroup, one work item per (row, halo cell)
template <typename T>
__global__ __launch_bounds__(kExt1dThreads) void k_ext1d_adj_fold(T* __restrict__ dst, const T* __restrict__ halo, int nr, int n, int F, int mode, int RB)
{
    const size_t row0 = (size_t)blockIdx.x * RB;
    const int rows = (size_t)nr - row0 < (size_t)RB ? (int)((size_t)nr - row0) : RB;
    const int H = adj_halo_len(n, F);
    const T* hl = halo + row0 * (size_t)H;
    __shared__ int hmap[2 * PDWT_MAX_FILTER_WIDTH];
    ext1d_halo_map<kExt1dThreads>(hmap, n, F, mode, (int)threadIdx.x);
    lds_barrier();
    ext1d_fold_halo<T, kExt1dThreads>(dst + row0 * (size_t)n, n, hl, hl + (F - 2), H, hmap, rows, n, F, (int)threadIdx.x);
}

// LDS of the fused form, in elements per row: the two line buffers of the forward transform (outputs of the odd levels | of the even
// levels) and one padded detail line
__host__ __device__ inline int adj1d_dof(int F) { return ext1d_ru4(F / 2 - 1); }
__host__ __device__ inline int adj1d_dstride(int N1, int F) { return ext1d_ru4(adj1d_dof(F) + N1 + F / 2 - 1); }

template <typename T, int HL>
__global__ __launch_bounds__(kExt1dThreads) void k_ext1d_adj_fused(T* __restrict__ dst, Ext1dBands<T> b, int Nr, int R, int mode, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = kExt1dThreads, off = ((HL - 2) + 3) & ~3, pad = HL / 2 - 1, dof = (pad + 3) & ~3;
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * R;
    const int rows = (size_t)Nr - row0 < (size_t)R ? (int)((size_t)Nr - row0) : R;
    const int L = b.nlev;
    T* buf[2];
    buf[0] = reinterpret_cast<T*>(smem);                        // R lines of stride(n_0): the outputs of levels 1, 3, ...
    buf[1] = buf[0] + (size_t)R * ext1d_stride(b.n[0], HL);     // R lines of stride(n_1): the outputs of levels 2, 4, ...
    T* db = buf[1] + (size_t)R * ext1d_stride(b.n[1], HL);      // R padded detail lines
    const int dstr = adj1d_dstride(b.n[1], HL);
    int* hmap = reinterpret_cast<int*>(db + (size_t)R * dstr);  // [2 HL - 3]: the targets of the halo cells of the level's output line
    T* cur = buf[L & 1];
    int cs = ext1d_stride(b.n[L], HL);
    ext1d_stage_rows<T, NT>(cur, cs, off, b.p[0] + row0 * (size_t)b.n[L], rows, b.n[L], tid);
    ext1d_zero_cells<T, NT>(cur, cs, off - pad, pad, rows, tid);
    ext1d_zero_cells<T, NT>(cur, cs, off + b.n[L], pad, rows, tid);
    for (int lev = L; lev >= 1; lev--) {
        const int N = b.n[lev], n = b.n[lev - 1], os = ext1d_stride(n, HL);
        ext1d_stage_rows<T, NT>(db, dstr, dof, b.p[lev] + row0 * (size_t)N, rows, N, tid);
        ext1d_zero_cells<T, NT>(db, dstr, dof - pad, pad, rows, tid);
        ext1d_zero_cells<T, NT>(db, dstr, dof + N, pad, rows, tid);
        ext1d_halo_map<NT>(hmap, n, HL, mode, tid);  // (the fold of the level before is behind a barrier)
        lds_barrier();
        T* out = buf[(lev - 1) & 1];
        ext1d_adj_level<T, HL, NT>(cur + off - pad, cs, db + dof - pad, dstr, out + off - (HL - 2), os, rows, N, HL, taps, tid);
        lds_barrier();
        ext1d_fold_halo<T, NT>(out + off, os, out + off - (HL - 2), out + off + n, os, hmap, rows, n, HL, tid);
        lds_barrier();
        if (lev == 1) {
            ext1d_store_rows<T, NT>(dst + row0 * (size_t)n, out, os, off, rows, n, tid);
            break;
        }
        // the folded line is the approximation cotangent of the next level: its padding (halo cells, read by the fold) is zeroed now;
        // the barrier after the staging of the next detail line orders this before the synthesis
        ext1d_zero_cells<T, NT>(out, os, off - pad, pad, rows, tid);
        ext1d_zero_cells<T, NT>(out, os, off + n, pad, rows, tid);
        cur = out, cs = os;
    }
}

// ---- geometry (host, no device) ---------------------------------------------------------------------------------------------------
// (external linkage: the 3-D adjoint, dwt_ext3d_adj.hip, refuses what this refuses with B = nz)
bool adj2_level_ok(long long B, int nr, int nc, int hlen)
{
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return false;
    if (B < 1 || B > kAdjMaxBatch) return false;
    if (nr < 1 || nc < 1 || nr < hlen - 1 || nc < hlen - 1 || nr > (1 << 30) || nc > (1 << 30)) return false;
    if ((unsigned long long)nr * (unsigned long long)nc >= (1ull << 31)) return false;
    // what the forward and inverse tile kernels take, and the rows of tiles of the extended grid
    if (idiv_up(ext_half(nr, hlen), TFY) > 65535 || idiv_up(nr, TIY) > 65535) return false;
    return idiv_up(adj_ext_len(nr, hlen), TIY) <= 65535;
}
static bool adj2_ok(long long B, int Nr, int Nc, int hlen, int levels)
{
    if (levels < 1 || levels > kAdjMaxLev) return false;
    for (int l = 0; l < levels; l++) {
        if (!adj2_level_ok(B, Nr, Nc, hlen)) return false;
        Nr = ext_half(Nr, hlen), Nc = ext_half(Nc, hlen);
    }
    return true;
}
// frame elements per image that any level of an Nr x Nc image needs at most (monotone in the sizes; a level's own need is adj_frame_elems)
static size_t adj2_frame_cap(int nr, int nc, int hlen) { return ((size_t)nr + 2 * hlen - 3) * ((size_t)nc + 2 * hlen - 3) - (size_t)nr * nc; }

static bool adj1_ok(long long nr, long long nc, int hlen)
{
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return false;
    if (nr < 1 || nc < 1 || nc < hlen - 1 || nc > (1 << 30)) return false;
    return (unsigned long long)nr * (unsigned long long)nc < (1ull << 31);
}
static bool adj1_levels_ok(int levels) { return levels >= 1 && levels <= kExt1dMaxLev; }

struct Adj1Plan {
    bool fused;
    int R;
    size_t lds;  // of a workgroup (R rows and the halo map)
};
constexpr size_t kAdj1MapBytes = sizeof(int) * 2 * PDWT_MAX_FILTER_WIDTH;
// The gate of pdwt_ext1d_fused AND the LDS of the adjoint pipeline (one padded detail line more than the forward) within a workgroup.
static Adj1Plan adj1_plan(int nc, int hlen, int levels, size_t elem)
{
    const int n1 = ext_half(nc, hlen);
    const size_t row = ((size_t)ext1d_stride(nc, hlen) + ext1d_stride(n1, hlen) + adj1d_dstride(n1, hlen)) * elem;
    Adj1Plan p{pdwt_ext1d_fused(nc, hlen, levels, (int)elem) == 1 && row + kAdj1MapBytes <= kLdsMax, 1, row + kAdj1MapBytes};
    if (!p.fused) return p;
    int R = 1;
    while (R < 64 && R * n1 < kExt1dThreads && 2 * R * row <= 32 * 1024) R *= 2;
    p.R = R, p.lds = R * row + kAdj1MapBytes;
    return p;
}

// ---- drivers -------------------------------------------------------------------------------------------------------------------
template <typename T, int HL>
static int launch_adj_syn(const AdjJob<T>& job, int B, const Taps2<T>& taps)
{
    constexpr size_t lds = tile_inv_lds<T, HL>(false);
    const dim3 grid(idiv_up(adj_ext_len(job.nc, HL), TIX), idiv_up(adj_ext_len(job.nr, HL), TIY), B);
    return launch_lds(k_ext_adj_syn<T, HL>, grid, dim3(kTileThreads), lds, job, taps);
}

// (external linkage: dwt_ext3d_adj.hip runs it on the nz planes of a volume)
template <typename T>
int adj2_forward_level(T* dst, const T* a, const T* h, const T* v, const T* d, int B, int nr, int nc, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!dst || !a || !h || !v || !d || !f || mode < 0 || mode >= EXT_NUM_MODES || !adj2_level_ok(B, nr, nc, f->hlen)) return PDWT_EINVAL;
    const int hlen = f->hlen;
    const bool fold = mode != EXT_ZERO && adj_frame_elems(nr, nc, hlen) > 0;
    if (fold && !tmp) return PDWT_EINVAL;
    const AdjJob<T> job{dst, {a, h, v, d}, fold ? tmp : nullptr, nr, nc, ext_half(nr, hlen), ext_half(nc, hlen), mode};
    const Taps2<T> taps = taps_adj<T>(f);
    if (const int rc = with_filter_length<2>(hlen, [&](auto hl) { return launch_adj_syn<T, decltype(hl)::value>(job, B, taps); }); rc != PDWT_OK) return rc;
    if (!fold) return PDWT_OK;
    AdjGap gap;
    adj_gap(nr, hlen, mode, gap.y0, gap.y1);
    adj_gap(nc, hlen, mode, gap.x0, gap.x1);
    hipLaunchKernelGGL((k_ext_adj_fold<T>), dim3(idiv_up(nc, AFX), idiv_up(nr, AFY), B), dim3(kAdjThreads), 0, stream(), dst, (const T*)tmp, nr, nc, hlen, mode, gap);
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

template int adj2_forward_level<float>(float*, const float*, const float*, const float*, const float*, int, int, int, int, const pdwt_filters_f32*, float*);
template int adj2_forward_level<double>(double*, const double*, const double*, const double*, const double*, int, int, int, int, const pdwt_filters_f64*, double*);

template <typename T>
static int adj2_forward(T* dst, T* const* c, int B, int Nr, int Nc, int levels, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!dst || !c || !f || !tmp || mode < 0 || mode >= EXT_NUM_MODES || !adj2_ok(B, Nr, Nc, f->hlen, levels)) return PDWT_EINVAL;
    for (int k = 0; k < 3 * levels + 1; k++)
        if (!c[k]) return PDWT_EINVAL;
    const int hlen = f->hlen;
    int nr[kAdjMaxLev + 1], nc[kAdjMaxLev + 1];
    nr[0] = Nr, nc[0] = Nc;
    for (int l = 1; l <= levels; l++) nr[l] = ext_half(nr[l - 1], hlen), nc[l] = ext_half(nc[l - 1], hlen);
    // scratch: the frame of a level | the two approximation cotangent stacks in turn
    const size_t stack1 = (size_t)B * nr[1] * nc[1];
    T* ping = tmp + (size_t)B * adj2_frame_cap(Nr, Nc, hlen);
    for (int l = levels; l >= 1; l--) {
        const T* a = l == levels ? c[0] : ping + ((l - 1) & 1) * stack1;
        T* out = l == 1 ? dst : ping + ((l - 2) & 1) * stack1;
        T* const* d = c + 3 * (l - 1) + 1;
        if (const int rc = adj2_forward_level<T>(out, a, d[0], d[1], d[2], B, nr[l - 1], nc[l - 1], mode, f, tmp); rc != PDWT_OK) return rc;
    }
    return PDWT_EXT2DB_LEVELS;
}

template <typename T>
static int adj1_forward_level(T* dst, const T* a, const T* d, int nr, int nc, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!dst || !a || !d || !f || mode < 0 || mode >= EXT_NUM_MODES || !adj1_ok(nr, nc, f->hlen)) return PDWT_EINVAL;
    const int hlen = f->hlen, N = ext_half(nc, hlen), H = adj_halo_len(nc, hlen);
    const bool fold = mode != EXT_ZERO && H > 0;
    if (fold && !tmp) return PDWT_EINVAL;
    const int tiles = idiv_up(N + hlen / 2 - 1, kExt1dTile);
    const size_t lds = sizeof(T) * 2 * (kExt1dTile + PDWT_MAX_FILTER_WIDTH / 2);
    hipLaunchKernelGGL((k_ext1d_adj<T>), dim3((unsigned)nr * (unsigned)tiles), dim3(kExt1dThreads), lds, stream(), dst, a, d, fold ? tmp : (T*)nullptr, nc, N, tiles,
                       hlen, taps_adj<T>(f));
    PDWT_HIP_TRY(hipGetLastError());
    if (!fold) return PDWT_OK;
    const int RB = std::max(1, kExt1dThreads / H);
    hipLaunchKernelGGL((k_ext1d_adj_fold<T>), dim3(idiv_up(nr, RB)), dim3(kExt1dThreads), 0, stream(), dst, (const T*)tmp, nr, nc, hlen, mode, RB);
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

template <typename T, int HL>
static int launch_adj1_fused(T* dst, const Ext1dBands<T>& b, int nr, int mode, const Adj1Plan& p, const Taps2<T>& taps)
{
    const int rc = launch_lds(k_ext1d_adj_fused<T, HL>, dim3(idiv_up(nr, p.R)), dim3(kExt1dThreads), p.lds, dst, b, nr, p.R, mode, taps);
    return rc == PDWT_OK ? PDWT_EXT1D_FUSED : rc;
}

template <typename T>
static int adj1_forward(T* dst, T* const* c, int nr, int nc, int levels, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!dst || !c || !f || mode < 0 || mode >= EXT_NUM_MODES || !adj1_levels_ok(levels) || !adj1_ok(nr, nc, f->hlen)) return PDWT_EINVAL;
    const int hlen = f->hlen;
    Ext1dBands<T> b;
    b.nlev = levels, b.n[0] = nc;
    for (int l = 1; l <= levels; l++) b.n[l] = ext_half(b.n[l - 1], hlen);
    for (int l = 0; l <= levels; l++) {
        if (!c[l]) return PDWT_EINVAL;
        b.p[l] = c[l];
    }
    const Adj1Plan p = adj1_plan(nc, hlen, levels, sizeof(T));
    if (p.fused) {
        const Taps2<T> taps = taps_adj<T>(f);
        return with_filter_length<2>(hlen, [&](auto hl) { return launch_adj1_fused<T, decltype(hl)::value>(dst, b, nr, mode, p, taps); });
    }
    if (!tmp) return PDWT_EINVAL;
    // scratch: the halo cells of a level | the two approximation cotangents in turn
    const size_t stack1 = (size_t)nr * b.n[1];
    T* ping = tmp + (size_t)nr * (2 * hlen - 3);
    for (int l = levels; l >= 1; l--) {
        const T* a = l == levels ? b.p[0] : ping + ((l - 1) & 1) * stack1;
        T* out = l == 1 ? dst : ping + ((l - 2) & 1) * stack1;
        if (const int rc = adj1_forward_level<T>(out, a, b.p[l], nr, b.n[l - 1], mode, f, tmp); rc != PDWT_OK) return rc;
    }
    return PDWT_EXT1D_LEVELS;
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
long long pdwt_ext2db_adjoint_tmp_elems(int B, int Nr, int Nc, int hlen, int levels, int elem_size)
{
    if (!adj2_ok(B, Nr, Nc, hlen, levels) || (elem_size != 4 && elem_size != 8)) return PDWT_EINVAL;
    const long long stack1 = (long long)B * ext_half(Nr, hlen) * ext_half(Nc, hlen);
    return (long long)B * (long long)adj2_frame_cap(Nr, Nc, hlen) + (levels > 1 ? 2 * stack1 : 0);
}
int pdwt_ext2db_forward_adjoint_level_f32(float* d_dst, const float* d_a, const float* d_h, const float* d_v, const float* d_d, int B, int nr, int nc, int mode,
                                          const pdwt_filters_f32* f, float* d_tmp)
{
    return adj2_forward_level<float>(d_dst, d_a, d_h, d_v, d_d, B, nr, nc, mode, f, d_tmp);
}
int pdwt_ext2db_forward_adjoint_level_f64(double* d_dst, const double* d_a, const double* d_h, const double* d_v, const double* d_d, int B, int nr, int nc, int mode,
                                          const pdwt_filters_f64* f, double* d_tmp)
{
    return adj2_forward_level<double>(d_dst, d_a, d_h, d_v, d_d, B, nr, nc, mode, f, d_tmp);
}
int pdwt_ext2db_forward_adjoint_f32(float* d_dst, float* const* d_coeffs, int B, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return adj2_forward<float>(d_dst, d_coeffs, B, Nr, Nc, levels, mode, f, d_tmp);
}
int pdwt_ext2db_forward_adjoint_f64(double* d_dst, double* const* d_coeffs, int B, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return adj2_forward<double>(d_dst, d_coeffs, B, Nr, Nc, levels, mode, f, d_tmp);
}
int pdwt_ext2db_inverse_adjoint_f32(const float* d_src, float* const* d_coeffs, int B, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp)
{
    pdwt_filters_f32 g;
    if (!adj_inverse_bank<float>(g, f)) return PDWT_EINVAL;
    return pdwt_ext2db_forward_f32(d_src, d_coeffs, B, Nr, Nc, levels, EXT_ZERO, &g, d_tmp);
}
int pdwt_ext2db_inverse_adjoint_f64(const double* d_src, double* const* d_coeffs, int B, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp)
{
    pdwt_filters_f64 g;
    if (!adj_inverse_bank<double>(g, f)) return PDWT_EINVAL;
    return pdwt_ext2db_forward_f64(d_src, d_coeffs, B, Nr, Nc, levels, EXT_ZERO, &g, d_tmp);
}

long long pdwt_ext1d_adjoint_tmp_elems(int Nr, int Nc, int hlen, int levels, int elem_size)
{
    if (!adj1_levels_ok(levels) || !adj1_ok(Nr, Nc, hlen) || (elem_size != 4 && elem_size != 8)) return PDWT_EINVAL;
    if (adj1_plan(Nc, hlen, levels, (size_t)elem_size).fused) return 0;
    return (long long)Nr * (2 * hlen - 3) + (levels > 1 ? 2ll * Nr * ext_half(Nc, hlen) : 0);
}
int pdwt_ext1d_forward_adjoint_level_f32(float* d_dst, const float* d_a, const float* d_d, int nr, int nc, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return adj1_forward_level<float>(d_dst, d_a, d_d, nr, nc, mode, f, d_tmp);
}
int pdwt_ext1d_forward_adjoint_level_f64(double* d_dst, const double* d_a, const double* d_d, int nr, int nc, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return adj1_forward_level<double>(d_dst, d_a, d_d, nr, nc, mode, f, d_tmp);
}
int pdwt_ext1d_forward_adjoint_f32(float* d_dst, float* const* d_coeffs, int nr, int nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return adj1_forward<float>(d_dst, d_coeffs, nr, nc, levels, mode, f, d_tmp);
}
int pdwt_ext1d_forward_adjoint_f64(double* d_dst, double* const* d_coeffs, int nr, int nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return adj1_forward<double>(d_dst, d_coeffs, nr, nc, levels, mode, f, d_tmp);
}
int pdwt_ext1d_inverse_adjoint_f32(const float* d_src, float* const* d_coeffs, int nr, int nc, int levels, const pdwt_filters_f32* f, float* d_tmp)
{
    pdwt_filters_f32 g;
    if (!adj_inverse_bank<float>(g, f)) return PDWT_EINVAL;
    return pdwt_ext1d_forward_f32(d_src, d_coeffs, nr, nc, levels, EXT_ZERO, &g, d_tmp);
}
int pdwt_ext1d_inverse_adjoint_f64(const double* d_src, double* const* d_coeffs, int nr, int nc, int levels, const pdwt_filters_f64* f, double* d_tmp)
{
    pdwt_filters_f64 g;
    if (!adj_inverse_bank<double>(g, f)) return PDWT_EINVAL;
    return pdwt_ext1d_forward_f64(d_src, d_coeffs, nr, nc, levels, EXT_ZERO, &g, d_tmp);
}
}
