// wpt2d.hip -- one depth of the 2-D wavelet packet transform (include/pdwt_hip.h "2-D wavelet packets").
//
// The packet tree decomposes EVERY band again: depth l holds 4^l equally sized nodes, contiguous in one array, node i with the
// children 4i + {0: A, 1: H, 2: V, 3: D} in the array of depth l + 1.  One depth step is therefore a batched one-level 2-D
// transform of small images, and runs in ONE launch: one workgroup per (tile, node), blockIdx.z = the position in the (optional)
// list of parent nodes.  The tile kernels are the x-y kernels of dwt3d.hip with a node in the place of a plane and the quadrants
// written straight to the children: stage the tile with its periodic halo in LDS, row pass into LDS, column pass out of it.
// Per output the taps run in the order of the checker's separable level, one FMA per tap (rows, then columns), so one level of
// a node has the arithmetic of the one-level 2-D transform of that node.  Haar (hlen 2) runs the clamped 2x2 butterfly of the
// reference's Haar level (src/haar.cu:10-58) instead.
// Traffic per depth and direction: one read of the parents (plus the tile halos) and one write of the children.
#include "vol3d.hpp"

namespace pdwt {

constexpr int kWpThreads = 256;
constexpr int WFX = 32, WFY = 16;  // forward tile (child positions)
constexpr int WIX = 64, WIY = 32;  // inverse tile (parent samples, even starts)
constexpr int kWpMaxNodes = 16384; // 4^7: the node count is a grid dimension

template <typename T>
struct WpJob {
    const T* src;      // forward: parents (node stride nr * nc); inverse: children (node stride hr * hc)
    T* dst;            // forward: children; inverse: parents
    const int* nodes;  // parent node of blockIdx.z, or nullptr: blockIdx.z itself
    int nr, nc, hr, hc;
};

template <typename T, int HL>
constexpr size_t wp_fwd_lds()
{
    return sizeof(T) * ((size_t)(2 * WFY + HL - 2) * (2 * WFX + HL - 2) + 2 * (size_t)(2 * WFY + HL - 2) * WFX);
}
template <typename T, int HL>
constexpr size_t wp_inv_lds()
{
    return sizeof(T) * (4 * (size_t)(WIY / 2 + HL / 2) * (WIX / 2 + HL / 2) + 2 * (size_t)WIY * (WIX / 2 + HL / 2));
}

// ---- forward: WFY x WFX positions of the four children of one parent node per workgroup ----------------------------------
template <typename T, int HL>
__global__ __launch_bounds__(kWpThreads) void k_wp_fwd(WpJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];  // (double: 8-byte alignment for either precision)
    constexpr int RI = 2 * WFY + HL - 2, CI = 2 * WFX + HL - 2, c = HL / 2 - 1;
    T* in = reinterpret_cast<T*>(smem_d);  // [RI][CI]
    T* rb = in + RI * CI;                  // [2][RI][WFX]: row pass lo | hi
    const int tid = threadIdx.x;
    const int node = job.nodes ? job.nodes[blockIdx.z] : (int)blockIdx.z;
    const int ox0 = blockIdx.x * WFX, oy0 = blockIdx.y * WFY;
    const int nc = job.nc, nr = job.nr;
    const T* __restrict__ parent = job.src + (size_t)node * nr * nc;
    const int gx0 = 2 * ox0 - c, gy0 = 2 * oy0 - c;
    for (int e = tid; e < RI * CI; e += kWpThreads) {
        const int r = e / CI, cc = e - r * CI;  // (compile-time divisor)
        in[e] = parent[(size_t)wrap_ext(gy0 + r, nr) * nc + wrap_ext(gx0 + cc, nc)];
    }
    __syncthreads();
    for (int e = tid; e < RI * WFX; e += kWpThreads) {
        const int r = e / WFX, ox = e % WFX;
        const T* p = in + r * CI + 2 * ox;
        const int z0 = opaque_zero();
        T sl = T(0), sh = T(0);
#pragma unroll
        for (int j = 0; j < HL; j++) {
            const T v = p[j];
            sl = fma_t<T>(v, taps.a[HL - 1 - j + z0], sl);
            sh = fma_t<T>(v, taps.b[HL - 1 - j + z0], sh);
        }
        rb[e] = sl;
        rb[RI * WFX + e] = sh;
    }
    __syncthreads();
    const size_t cs = (size_t)job.hr * job.hc;  // child stride
    T* __restrict__ child = job.dst + 4 * (size_t)node * cs;
    for (int e = tid; e < WFY * WFX; e += kWpThreads) {
        const int oy = e / WFX, ox = e % WFX;
        if (oy0 + oy >= job.hr || ox0 + ox >= job.hc) continue;
        const size_t o = (size_t)(oy0 + oy) * job.hc + (ox0 + ox);
#pragma unroll
        for (int xb = 0; xb < 2; xb++) {  // row low: A (column low), H (column high); row high: V, D
            const T* p = rb + xb * RI * WFX + (2 * oy) * WFX + ox;
            const int z0 = opaque_zero();
            T sl = T(0), sh = T(0);
#pragma unroll
            for (int j = 0; j < HL; j++) {
                const T v = p[j * WFX];
                sl = fma_t<T>(v, taps.a[HL - 1 - j + z0], sl);
                sh = fma_t<T>(v, taps.b[HL - 1 - j + z0], sh);
            }
            child[(2 * xb) * cs + o] = sl;
            child[(2 * xb + 1) * cs + o] = sh;
        }
    }
}

// ---- inverse: WIY x WIX samples of one parent node per workgroup ----------------------------------------------------------
// Stages the window of the four children the tile needs (wrap_per), runs the synthesis along the columns into an LDS buffer
// ((A, H) | (V, D)), then along the rows into the parent.  The oracle's syn_lines rule, the two branch sums added once.
template <typename T, int HL>
__global__ __launch_bounds__(kWpThreads) void k_wp_inv(WpJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];
    constexpr int h2 = HL / 2, c = h2 / 2, shift = (h2 & 1) ? 0 : 1;
    constexpr int WR = WIY / 2 + h2, WC = WIX / 2 + h2;
    T* in = reinterpret_cast<T*>(smem_d);  // [4][WR][WC]
    T* cb = in + 4 * WR * WC;              // [2][WIY][WC]
    const int tid = threadIdx.x;
    const int node = job.nodes ? job.nodes[blockIdx.z] : (int)blockIdx.z;
    const int g0x = blockIdx.x * WIX, g0y = blockIdx.y * WIY;  // even
    const int hc = job.hc, hr = job.hr;
    const int wx0 = g0x / 2 - c, wy0 = g0y / 2 - c;
    const size_t cs = (size_t)hr * hc;
    const T* __restrict__ child = job.src + 4 * (size_t)node * cs;
    for (int e = tid; e < 4 * WR * WC; e += kWpThreads) {
        const int qd = e / (WR * WC), rem = e - qd * (WR * WC), r = rem / WC, cc = rem - r * WC;
        in[e] = child[qd * cs + (size_t)wrap_per(wy0 + r, hr) * hc + wrap_per(wx0 + cc, hc)];
    }
    __syncthreads();
    for (int e = tid; e < 2 * WIY * WC; e += kWpThreads) {
        const int xb = e / (WIY * WC), rem = e - xb * (WIY * WC), gy = rem / WC, cc = rem - gy * WC;
        const int gp = gy + shift, lp = gp >> 1;
        const bool odd_tap = (gp & 1) == 0;
        const T* pa = in + (2 * xb) * WR * WC + lp * WC + cc;
        const T* pd = pa + WR * WC;
        T sa = T(0), sd = T(0);
#pragma unroll
        for (int j = 0; j < h2; j++) {
            const T fl = odd_tap ? taps.a[HL - 2 - 2 * j] : taps.a[HL - 1 - 2 * j];
            const T fh = odd_tap ? taps.b[HL - 2 - 2 * j] : taps.b[HL - 1 - 2 * j];
            sa = fma_t<T>(pa[j * WC], fl, sa);
            sd = fma_t<T>(pd[j * WC], fh, sd);
        }
        cb[e] = sa + sd;
    }
    __syncthreads();
    const int nc = job.nc, nr = job.nr;
    T* __restrict__ parent = job.dst + (size_t)node * nr * nc;
    for (int e = tid; e < WIY * WIX; e += kWpThreads) {
        const int gy = e / WIX, gx = e % WIX;
        if (g0y + gy >= nr || g0x + gx >= nc) continue;
        const int gp = gx + shift, lp = gp >> 1;
        const bool odd_tap = (gp & 1) == 0;
        const T* pa = cb + gy * WC + lp;
        const T* pd = pa + WIY * WC;
        T sa = T(0), sd = T(0);
#pragma unroll
        for (int j = 0; j < h2; j++) {
            const T fl = odd_tap ? taps.a[HL - 2 - 2 * j] : taps.a[HL - 1 - 2 * j];
            const T fh = odd_tap ? taps.b[HL - 2 - 2 * j] : taps.b[HL - 1 - 2 * j];
            sa = fma_t<T>(pa[j], fl, sa);
            sd = fma_t<T>(pd[j], fh, sd);
        }
        parent[(size_t)(g0y + gy) * nc + (g0x + gx)] = sa + sd;
    }
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
    const size_t lds = fwd ? wp_fwd_lds<T, HL>() : wp_inv_lds<T, HL>();
    const void* kfn = fwd ? (const void*)k_wp_fwd<T, HL> : (const void*)k_wp_inv<T, HL>;
    if (lds > 64 * 1024)
        if (const int rc = lds_opt_in_ptr(kfn); rc != PDWT_OK) return rc;
    if (fwd) hipLaunchKernelGGL((k_wp_fwd<T, HL>), dim3(idiv_up(job.hc, WFX), idiv_up(job.hr, WFY), nnodes), dim3(kWpThreads), lds, stream(), job, taps);
    else hipLaunchKernelGGL((k_wp_inv<T, HL>), dim3(idiv_up(job.nc, WIX), idiv_up(job.nr, WIY), nnodes), dim3(kWpThreads), lds, stream(), job, taps);
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
    const int tile_rows = hlen == 2 ? (dir == 0 ? idiv_up(job.hr, 4) : idiv_up(nr, 4)) : (dir == 0 ? idiv_up(job.hr, WFY) : idiv_up(nr, WIY));
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
