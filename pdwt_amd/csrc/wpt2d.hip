// wpt2d.hip -- one depth of the 2-D wavelet packet transform (include/pdwt_hip.h "2-D wavelet packets").
//
// The packet tree decomposes EVERY band again: depth l holds 4^l equally sized nodes, contiguous in one array, node i with the
// children 4i + {0: A, 1: H, 2: V, 3: D} in the array of depth l + 1.  One depth step is therefore a batched one-level 2-D
// transform of small images, and runs in ONE launch: one workgroup per (tile, node), blockIdx.z = the position in the (optional)
// list of parent nodes.  The tile kernels are the x-y kernels of dwt3d.hip with a node in the place of a plane and the quadrants
// written straight to the children: stage the tile with its periodic halo in LDS, row pass into LDS, column pass out of it -- the
// stages of tile_stages.hpp, which both files call; the kernels here only place the node and its children.
// Per output the taps run in the order of the checker's separable level, one FMA per tap (rows, then columns), so one level of
// a node has the arithmetic of the one-level 2-D transform of that node.  Haar (hlen 2) runs the clamped 2x2 butterfly of the
// reference's Haar level (src/haar.cu:10-58) instead.
// Traffic per depth and direction: one read of the parents (plus the tile halos) and one write of the children.
#include "tile_stages.hpp"

namespace pdwt {

constexpr int kWpThreads = 256;    // the Haar and cost kernels (the tile kernels: kTileThreads)
// The tile of tile_stages.hpp.  (tests/test_newer_bank_matrix_cpu.py reads these four from this file; the kernels use the shared constants.)
constexpr int WFX = 32, WFY = 16, WIX = 64, WIY = 32;
static_assert(WFX == TFX && WFY == TFY && WIX == TIX && WIY == TIY, "the tile shape is defined in tile_stages.hpp");
constexpr int kWpMaxNodes = 16384; // 4^7: the node count is a grid dimension

template <typename T>
struct WpJob {
    const T* src;      // forward: parents (node stride nr * nc); inverse: children (node stride hr * hc)
    T* dst;            // forward: children; inverse: parents
    const int* nodes;  // parent node of blockIdx.z, or nullptr: blockIdx.z itself
    int nr, nc, hr, hc;
};

// ---- forward: TFY x TFX positions of the four children of one parent node per workgroup ----------------------------------
template <typename T, int HL>
__global__ __launch_bounds__(kTileThreads) void k_wp_fwd(WpJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];  // (double: 8-byte alignment for either precision)
    constexpr int RI = tile_fwd_win(TFY, HL), CI = tile_fwd_win(TFX, HL), c = HL / 2 - 1;
    T* in = reinterpret_cast<T*>(smem_d);  // [RI][CI]
    T* rb = in + RI * CI;                  // [2][RI][TFX]: row pass lo | hi
    const int tid = threadIdx.x;
    const int node = job.nodes ? job.nodes[blockIdx.z] : (int)blockIdx.z;
    const int ox0 = blockIdx.x * TFX, oy0 = blockIdx.y * TFY;
    const size_t cs = (size_t)job.hr * job.hc;  // child stride
    T* child = job.dst + 4 * (size_t)node * cs;  // A, H, V, D = children 4 node + 0 .. 3
    tile_stage_window_per<T, RI, CI, kTileThreads>(in, job.src + (size_t)node * job.nr * job.nc, job.nr, job.nc, 2 * oy0 - c, 2 * ox0 - c, tid);
    tile_rows_analysis<T, HL, RI, CI, TFX, kTileThreads>(in, rb, taps, tid);
    tile_cols_analysis_write<T, HL, RI, TFX, TFY, kTileThreads>(rb, taps, child, child + cs, child + 2 * cs, child + 3 * cs, job.hr, job.hc, oy0, ox0, tid);
}

// ---- inverse: TIY x TIX samples of one parent node per workgroup ----------------------------------------------------------
// The four child windows staged with wrap_per, synthesis along the columns into LDS ((A, H) | (V, D)), then along the rows into the
// parent: the oracle's syn_lines rule (the stages of tile_stages.hpp with the shift of the periodised synthesis).
template <typename T, int HL>
__global__ __launch_bounds__(kTileThreads) void k_wp_inv(WpJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];
    constexpr int c = HL / 4, SH = syn_shift(HL);
    constexpr int WR = tile_inv_win(TIY, HL, true), WC = tile_inv_win(TIX, HL, true);
    T* in = reinterpret_cast<T*>(smem_d);  // [4][WR][WC]
    T* cb = in + 4 * WR * WC;              // [2][TIY][WC]
    const int tid = threadIdx.x;
    const int node = job.nodes ? job.nodes[blockIdx.z] : (int)blockIdx.z;
    const int g0x = blockIdx.x * TIX, g0y = blockIdx.y * TIY;  // even
    const size_t cs = (size_t)job.hr * job.hc;
    const T* child = job.src + 4 * (size_t)node * cs;
    tile_stage_children_per<T, WR, WC, kTileThreads>(in, [=](int qd) { return child + qd * cs; }, job.hr, job.hc, g0y / 2 - c, g0x / 2 - c, tid);
    tile_cols_synthesis<T, HL, SH, WR, WC, TIY, kTileThreads>(in, cb, taps, tid);
    tile_rows_synthesis_write<T, HL, SH, WC, TIY, TIX, kTileThreads>(cb, taps, job.dst + (size_t)node * job.nr * job.nc, job.nr, job.nc, g0y, g0x, tid);
}

// ---- Haar: the clamped 2x2 butterfly, one thread per child position / parent sample ----------------------------------------
//   a=x[2y,2x] b=x[2y,2x+1] c=x[2y+1,2x] d=x[2y+1,2x+1], the odd index clamped to the last row / column (no wrap)
//   A=.5((a+c)+(b+d))  V=.5((a+c)-(b+d))  H=.5((a-c)+(b-d))  D=.5((a-c)-(b-d))
template <typename T>
__global__ __launch_bounds__(kWpThreads) void k_wp_haar_fwd(WpJob<T> job)
{
    const int node = job.nodes ? job.nodes[blockIdx.z] : (int)blockIdx.z;
    const int xx = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (xx >= job.hc || y >= job.hr) return;
    const int nr = job.nr, nc = job.nc;
    const T* __restrict__ x = job.src + (size_t)node * nr * nc;
    const int y0 = 2 * y, y1 = (2 * y + 1 == nr) ? nr - 1 : 2 * y + 1;
    const int x0 = 2 * xx, x1 = (2 * xx + 1 == nc) ? nc - 1 : 2 * xx + 1;
    const T a = x[(size_t)y0 * nc + x0], b = x[(size_t)y0 * nc + x1];
    const T cc = x[(size_t)y1 * nc + x0], d = x[(size_t)y1 * nc + x1];
    const size_t cs = (size_t)job.hr * job.hc, o = (size_t)y * job.hc + xx;
    T* __restrict__ child = job.dst + 4 * (size_t)node * cs;
    child[o] = T(0.5) * ((a + cc) + (b + d));
    child[cs + o] = T(0.5) * ((a - cc) + (b - d));
    child[2 * cs + o] = T(0.5) * ((a + cc) - (b + d));
    child[3 * cs + o] = T(0.5) * ((a - cc) - (b - d));
}

template <typename T>
__global__ __launch_bounds__(kWpThreads) void k_wp_haar_inv(WpJob<T> job)
{
    const int node = job.nodes ? job.nodes[blockIdx.z] : (int)blockIdx.z;
    const int xx = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (xx >= job.nc || y >= job.nr) return;
    const size_t cs = (size_t)job.hr * job.hc, o = (size_t)(y >> 1) * job.hc + (xx >> 1);
    const T* __restrict__ child = job.src + 4 * (size_t)node * cs;
    const T a = child[o], cc = child[cs + o], b = child[2 * cs + o], d = child[3 * cs + o];
    T r;
    if (!(y & 1)) r = (xx & 1) ? T(0.5) * ((a + cc) - (b + d)) : T(0.5) * ((a + cc) + (b + d));
    else r = (xx & 1) ? T(0.5) * ((a - cc) - (b - d)) : T(0.5) * ((a - cc) + (b - d));
    job.dst[(size_t)node * job.nr * job.nc + (size_t)y * job.nc + xx] = r;
}

// ---- additive node costs ---------------------------------------------------------------------------------------------------
// blockIdx.y = node, blockIdx.x = chunk of the node: every thread adds its elements (stride = the threads of the node's chunks)
// in double, the workgroup combines its 256 sums in a fixed order (wave shuffles, then the 4 waves in LDS) and stores ONE partial
// per (node, chunk).  The entry point adds the chunks of a node in chunk order on the host: no atomics, two runs give the same bits.
//   kind 0 ("l1"): sum |c|     kind 1 ("shannon"): -sum c^2 ln c^2, zero terms skipped
constexpr int kCostChunkElems = 8192;
constexpr int kCostMaxChunks = 128;

template <typename T>
__global__ __launch_bounds__(kWpThreads) void k_wp_cost(const T* __restrict__ nodes, size_t node_elems, int kind, double* __restrict__ partial)
{
    __shared__ double wsum[kWpThreads / 64];
    const T* __restrict__ x = nodes + (size_t)blockIdx.y * node_elems;
    const size_t stride = (size_t)gridDim.x * kWpThreads;
    double s = 0.0;
    if (kind == 0) {
        for (size_t e = (size_t)blockIdx.x * kWpThreads + threadIdx.x; e < node_elems; e += stride) s += fabs((double)x[e]);
    } else {
        for (size_t e = (size_t)blockIdx.x * kWpThreads + threadIdx.x; e < node_elems; e += stride) {
            const double v = (double)x[e], v2 = v * v;
            if (v2 > 0.0) s -= v2 * log(v2);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// ---- drivers -----------------------------------------------------------------------------------------------------------------
template <typename T, int HL>
static int launch_wp(int dir, const WpJob<T>& job, int nnodes, const Taps2<T>& taps)
{
    const bool fwd = dir == 0;
    const size_t lds = fwd ? tile_fwd_lds<T, HL>(false) : tile_inv_lds<T, HL>(true);
    const void* kfn = fwd ? (const void*)k_wp_fwd<T, HL> : (const void*)k_wp_inv<T, HL>;
    if (lds > 64 * 1024)
        if (const int rc = lds_opt_in_ptr(kfn); rc != PDWT_OK) return rc;
    if (fwd) hipLaunchKernelGGL((k_wp_fwd<T, HL>), dim3(idiv_up(job.hc, TFX), idiv_up(job.hr, TFY), nnodes), dim3(kTileThreads), lds, stream(), job, taps);
    else hipLaunchKernelGGL((k_wp_inv<T, HL>), dim3(idiv_up(job.nc, TIX), idiv_up(job.nr, TIY), nnodes), dim3(kTileThreads), lds, stream(), job, taps);
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

// dir 0: parents -> children; dir 1: children -> parents
template <typename T>
static int wp_level(int dir, const T* src, T* dst, int nr, int nc, const int* d_nodes, int nnodes, const typename FiltersOf<T>::type* f)
{
    if (!src || !dst || !f || nr < 1 || nc < 1 || nnodes < 1 || nnodes > kWpMaxNodes) return PDWT_EINVAL;
    const int hlen = f->hlen;
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return PDWT_EINVAL;
    if (hlen > 2 && (nr < hlen || nc < hlen)) return PDWT_EINVAL;  // a node smaller than the bank
    if ((unsigned long long)nr * (unsigned long long)nc >= (1ull << 31)) return PDWT_EINVAL;
    WpJob<T> job{};
    job.src = src, job.dst = dst, job.nodes = d_nodes;
    job.nr = nr, job.nc = nc, job.hr = div2(nr), job.hc = div2(nc);
    // rows of tiles are a grid dimension too: refused here, before anything is launched
    const int tile_rows = hlen == 2 ? (dir == 0 ? idiv_up(job.hr, 4) : idiv_up(nr, 4)) : (dir == 0 ? idiv_up(job.hr, TFY) : idiv_up(nr, TIY));
    if (tile_rows > 65535) return PDWT_EINVAL;
    if (hlen == 2) {
        const dim3 grid = dir == 0 ? dim3(idiv_up(job.hc, 64), tile_rows, nnodes) : dim3(idiv_up(nc, 64), tile_rows, nnodes);
        if (dir == 0) hipLaunchKernelGGL((k_wp_haar_fwd<T>), grid, dim3(kWpThreads), 0, stream(), job);
        else hipLaunchKernelGGL((k_wp_haar_inv<T>), grid, dim3(kWpThreads), 0, stream(), job);
        PDWT_HIP_TRY(hipGetLastError());
        return PDWT_OK;
    }
    const Taps2<T> taps = dir == 0 ? taps_fwd<T>(f) : taps_inv<T>(f);
    return with_filter_length<4>(hlen, [&](auto hl) { return launch_wp<T, decltype(hl)::value>(dir, job, nnodes, taps); });
}

template <typename T>
static int wp_cost(const T* d_nodes, size_t node_elems, int nnodes, int kind, double* out)
{
    if (!d_nodes || !out || node_elems < 1 || nnodes < 1 || nnodes > 65535 || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    size_t nch = (node_elems + kCostChunkElems - 1) / kCostChunkElems;
    if (nch > (size_t)kCostMaxChunks) nch = kCostMaxChunks;
    const size_t np = (size_t)nnodes * nch;
    double* d_part = (double*)pdwt_malloc(np * sizeof(double));
    if (!d_part) return PDWT_ENOMEM;
    double* h_part = (double*)malloc(np * sizeof(double));
    if (!h_part) {
        (void)pdwt_free(d_part);
        return PDWT_ENOMEM;
    }
    hipLaunchKernelGGL((k_wp_cost<T>), dim3((unsigned)nch, (unsigned)nnodes), dim3(kWpThreads), 0, stream(), d_nodes, node_elems, kind, d_part);
    int rc = hipGetLastError() == hipSuccess ? PDWT_OK : PDWT_EHIP;
    if (rc == PDWT_OK) rc = pdwt_memcpy_d2h(h_part, d_part, np * sizeof(double));  // (synchronises)
    if (rc == PDWT_OK)
        for (int i = 0; i < nnodes; i++) {
            double s = 0.0;
            for (size_t k = 0; k < nch; k++) s += h_part[(size_t)i * nch + k];
            out[i] = s;
        }
    free(h_part);
    const int rf = pdwt_free(d_part);
    return rc != PDWT_OK ? rc : rf;
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_wpt2d_forward_level_f32(const float* d_parent, float* d_child, int nr, int nc, const int* d_nodes, int nnodes, const pdwt_filters_f32* f)
{
    return wp_level<float>(0, d_parent, d_child, nr, nc, d_nodes, nnodes, f);
}
int pdwt_wpt2d_forward_level_f64(const double* d_parent, double* d_child, int nr, int nc, const int* d_nodes, int nnodes, const pdwt_filters_f64* f)
{
    return wp_level<double>(0, d_parent, d_child, nr, nc, d_nodes, nnodes, f);
}
int pdwt_wpt2d_inverse_level_f32(float* d_parent, const float* d_child, int nr, int nc, const int* d_nodes, int nnodes, const pdwt_filters_f32* f)
{
    return wp_level<float>(1, d_child, d_parent, nr, nc, d_nodes, nnodes, f);
}
int pdwt_wpt2d_inverse_level_f64(double* d_parent, const double* d_child, int nr, int nc, const int* d_nodes, int nnodes, const pdwt_filters_f64* f)
{
    return wp_level<double>(1, d_child, d_parent, nr, nc, d_nodes, nnodes, f);
}
int pdwt_wpt2d_node_cost_f32(const float* d_nodes, size_t node_elems, int nnodes, int kind, double* out) { return wp_cost<float>(d_nodes, node_elems, nnodes, kind, out); }
int pdwt_wpt2d_node_cost_f64(const double* d_nodes, size_t node_elems, int nnodes, int kind, double* out) { return wp_cost<double>(d_nodes, node_elems, nnodes, kind, out); }
}
