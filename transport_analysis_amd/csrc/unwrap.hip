// unwrap.hip — undo periodic wrapping of a staged float64 pair-major position slab in place (MDAnalysis' NoJump,
// Kulke & Vermaas, JCTC 2022, eq. B6), over the staged frames in order:
//
//   f(t) = x(t) H(t)^-1,   n(0) = 0,   n(t) = n(t-1) + rint(f(t) - f(t-1)),   x_u(t) = x(t) - n(t) H(t)
//
// with H(t) the box of frame t (rows = box vectors; unwrap_box.hpp builds the table on the host).  n is an integer
// 3-vector per atom, so its prefix sum along time is exact and independent of the order of the additions: the pass reads
// the slab once, writes it once, needs no atomics and gives the same bits from run to run.  Frame 0 (n = 0) is written
// back as it was read.  rint is round-half-even, as np.round.
//
// A wave walks one unit of columns along time in chunks of 256 frames, a lane owning four consecutive frames (16-byte
// rows of each column pair): the per-frame jumps rint(df) and their lane-local prefix, a wave-wide scan of the lane
// totals (__shfl_up), the running count and the last f carried into the next chunk from lane 63.  Rows n_frames ...
// pitch - 1 and the partner of an unpaired last column are never written (the FFT kernels read them as zero padding).
//   k_unwrap_ortho : orthogonal boxes, one wave per column pair; column c is box axis axes[c % D], so the two columns
//                    of a pair may belong to different axes or atoms.
//   k_unwrap_tric  : any box, D = 3: one wave per two atoms = three pairs (an odd last atom: one pair and a half).
// Both read the box table at frame t (per-frame boxes) or at 0 (a constant box: one address for the whole wave).
#include <hip/hip_runtime.h>

#include "ta_internal.hpp"
#include "unwrap_box.hpp"

namespace ta {
namespace {

constexpr int kUnwrapThreads = 256, kRows = 4, kChunk = 64 * kRows;

template <bool kPerFrame>
__device__ inline double box_at(const double* __restrict__ tab, long tpitch, int row, long t) {
    return tab[row * tpitch + (kPerFrame ? t : 0)];
}

// wave-wide inclusive scan of NC lane totals, in place
template <int NC>
__device__ inline void wave_scan(int (&s)[NC], int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int u = __shfl_up(s[c], o, 64);
            if (lane >= o) s[c] += u;
        }
    }
}

// The common step of both kernels for NC columns of one chunk: f[c][i] = the fractional coordinate of column c at frame
// tb + i (lanes: tb = t0 + 4 lane); prev[c] = f of the frame before the chunk.  Out: n[c][i] = the image count at
// frame tb + i, after which n_carry / prev hold the values at the chunk's last frame.
template <int NC>
__device__ inline void count_images(const double (&f)[NC][kRows], long tb, long T, int lane, double (&prev)[NC],
                                    int (&n_carry)[NC], int (&n)[NC][kRows]) {
    int tot[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double up = __shfl_up(f[c][kRows - 1], 1, 64);
        double p = lane ? up : prev[c];
        int acc = 0;
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            acc += tb + i < T ? (int)rint(f[c][i] - p) : 0;
            n[c][i] = acc;  // lane-local inclusive prefix
            p = f[c][i];
        }
        tot[c] = acc;
    }
    wave_scan<NC>(tot, lane);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int before = n_carry[c] + tot[c] - n[c][kRows - 1];  // carry + the lanes below
#pragma unroll
        for (int i = 0; i < kRows; ++i) n[c][i] += before;
        n_carry[c] += __shfl(tot[c], 63, 64);
        prev[c] = __shfl(f[c][kRows - 1], 63, 64);
    }
}

template <bool kPerFrame>
__global__ void __launch_bounds__(kUnwrapThreads)
    k_unwrap_ortho(double* __restrict__ slab, long pitch, long T, long n_cols, int D, int axes_packed,
                   const double* __restrict__ tab, long tpitch) {
    const int lane = threadIdx.x & 63;
    const long pair = (long)blockIdx.x * (kUnwrapThreads / 64) + (threadIdx.x >> 6);
    if (pair >= (n_cols + 1) / 2) return;  // (a whole wave)
    const long c0 = 2 * pair;
    const bool two = c0 + 1 < n_cols;
    const int a0 = (axes_packed >> (2 * (int)(c0 % D))) & 3;
    const int a1 = two ? (axes_packed >> (2 * (int)((c0 + 1) % D))) & 3 : a0;
    const int h0 = diag_row(a0), h1 = diag_row(a1), m0 = 6 + h0, m1 = 6 + h1;
    double2* x = reinterpret_cast<double2*>(slab) + pair * pitch;
    const double2 x0 = x[0];
    double prev[2] = {x0.x * box_at<kPerFrame>(tab, tpitch, m0, 0), x0.y * box_at<kPerFrame>(tab, tpitch, m1, 0)};
    int carry[2] = {0, 0};
    for (long t0 = 0; t0 < T; t0 += kChunk) {
        const long tb = t0 + kRows * lane;
        double2 r[kRows];
        double f[2][kRows];
#pragma unroll
        for (int i = 0; i < kRows; ++i) r[i] = tb + i < T ? x[tb + i] : double2{0.0, 0.0};
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            const long t = tb + i < T ? tb + i : 0;
            f[0][i] = r[i].x * box_at<kPerFrame>(tab, tpitch, m0, t);
            f[1][i] = r[i].y * box_at<kPerFrame>(tab, tpitch, m1, t);
        }
        int n[2][kRows];
        count_images<2>(f, tb, T, lane, prev, carry, n);
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            const long t = tb + i;
            if (t >= T) continue;
            const double u = r[i].x - (double)n[0][i] * box_at<kPerFrame>(tab, tpitch, h0, t);
            if (two) x[t] = double2{u, r[i].y - (double)n[1][i] * box_at<kPerFrame>(tab, tpitch, h1, t)};
            else reinterpret_cast<double*>(x + t)[0] = u;  // the partner column stays untouched
        }
    }
}

template <bool kPerFrame>
__global__ void __launch_bounds__(kUnwrapThreads)
    k_unwrap_tric(double* __restrict__ slab, long pitch, long T, long n_atoms, const double* __restrict__ tab, long tpitch) {
    const int lane = threadIdx.x & 63;
    const long a = 2 * ((long)blockIdx.x * (kUnwrapThreads / 64) + (threadIdx.x >> 6));  // atoms a, a + 1
    if (a >= n_atoms) return;  // (a whole wave)
    const bool two = a + 1 < n_atoms;
    // columns 3a ... 3a + 5 = pairs 3a/2 ... 3a/2 + 2: (A0 A1) (A2 B0) (B1 B2); an odd last atom has (A0 A1) (A2 0)
    double2* p = reinterpret_cast<double2*>(slab) + (3 * a / 2) * pitch;
    double prev[6];
    {
        const double2 u = p[0], v = p[pitch], w = two ? p[2 * pitch] : double2{0.0, 0.0};
        const double xa[3] = {u.x, u.y, v.x}, xb[3] = {v.y, w.x, w.y};
        const double* xs[2] = {xa, xb};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double* y = xs[k];
            prev[3 * k + 0] = y[0] * box_at<kPerFrame>(tab, tpitch, 6, 0) + y[1] * box_at<kPerFrame>(tab, tpitch, 7, 0) +
                              y[2] * box_at<kPerFrame>(tab, tpitch, 9, 0);
            prev[3 * k + 1] = y[1] * box_at<kPerFrame>(tab, tpitch, 8, 0) + y[2] * box_at<kPerFrame>(tab, tpitch, 10, 0);
            prev[3 * k + 2] = y[2] * box_at<kPerFrame>(tab, tpitch, 11, 0);
        }
    }
    int carry[6] = {0, 0, 0, 0, 0, 0};
    for (long t0 = 0; t0 < T; t0 += kChunk) {
        const long tb = t0 + kRows * lane;
        double xv[6][kRows], f[6][kRows];
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            const long t = tb + i;
            const bool in = t < T;
            const double2 u = in ? p[t] : double2{0.0, 0.0};
            const double2 v = in ? p[pitch + t] : double2{0.0, 0.0};
            const double2 w = in && two ? p[2 * pitch + t] : double2{0.0, 0.0};
            xv[0][i] = u.x, xv[1][i] = u.y, xv[2][i] = v.x, xv[3][i] = v.y, xv[4][i] = w.x, xv[5][i] = w.y;
            const long tt = in ? t : 0;
            const double m00 = box_at<kPerFrame>(tab, tpitch, 6, tt), m10 = box_at<kPerFrame>(tab, tpitch, 7, tt);
            const double m11 = box_at<kPerFrame>(tab, tpitch, 8, tt), m20 = box_at<kPerFrame>(tab, tpitch, 9, tt);
            const double m21 = box_at<kPerFrame>(tab, tpitch, 10, tt), m22 = box_at<kPerFrame>(tab, tpitch, 11, tt);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double y0 = xv[3 * k][i], y1 = xv[3 * k + 1][i], y2 = xv[3 * k + 2][i];
                f[3 * k + 0][i] = y0 * m00 + y1 * m10 + y2 * m20;
                f[3 * k + 1][i] = y1 * m11 + y2 * m21;
                f[3 * k + 2][i] = y2 * m22;
            }
        }
        int n[6][kRows];
        count_images<6>(f, tb, T, lane, prev, carry, n);
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            const long t = tb + i;
            if (t >= T) continue;
            const double h00 = box_at<kPerFrame>(tab, tpitch, 0, t), h10 = box_at<kPerFrame>(tab, tpitch, 1, t);
            const double h11 = box_at<kPerFrame>(tab, tpitch, 2, t), h20 = box_at<kPerFrame>(tab, tpitch, 3, t);
            const double h21 = box_at<kPerFrame>(tab, tpitch, 4, t), h22 = box_at<kPerFrame>(tab, tpitch, 5, t);
            double o[6];
#pragma unroll
            for (int k = 0; k < 2; ++k) {  // x - n H, n a row vector
                const double n0 = (double)n[3 * k][i], n1 = (double)n[3 * k + 1][i], n2 = (double)n[3 * k + 2][i];
                o[3 * k + 0] = xv[3 * k + 0][i] - (n0 * h00 + n1 * h10 + n2 * h20);
                o[3 * k + 1] = xv[3 * k + 1][i] - (n1 * h11 + n2 * h21);
                o[3 * k + 2] = xv[3 * k + 2][i] - n2 * h22;
            }
            p[t] = double2{o[0], o[1]};
            if (two) {
                p[pitch + t] = double2{o[2], o[3]};
                p[2 * pitch + t] = double2{o[4], o[5]};
            } else {
                reinterpret_cast<double*>(p + pitch + t)[0] = o[2];  // the partner column stays untouched
            }
        }
    }
}

}  // namespace

hipError_t launch_unwrap(double* slab, long pitch, long T, long n_atoms, int D, const int* axes, bool triclinic,
                         bool per_frame, const double* d_tab, long tpitch, hipStream_t st) {
    if (D < 1 || D > 3 || (triclinic && D != 3)) return hipErrorInvalidValue;
    const int wpg = kUnwrapThreads / 64;
    if (triclinic) {
        const long units = (n_atoms + 1) / 2;
        const dim3 grid((unsigned)((units + wpg - 1) / wpg));
        if (per_frame) hipLaunchKernelGGL(k_unwrap_tric<true>, grid, dim3(kUnwrapThreads), 0, st, slab, pitch, T, n_atoms, d_tab, tpitch);
        else hipLaunchKernelGGL(k_unwrap_tric<false>, grid, dim3(kUnwrapThreads), 0, st, slab, pitch, T, n_atoms, d_tab, tpitch);
        return hipGetLastError();
    }
    int packed = 0;
    for (int d = 0; d < D; ++d) packed |= (axes[d] & 3) << (2 * d);
    const long n_cols = n_atoms * D, units = (n_cols + 1) / 2;
    const dim3 grid((unsigned)((units + wpg - 1) / wpg));
    if (per_frame)
        hipLaunchKernelGGL(k_unwrap_ortho<true>, grid, dim3(kUnwrapThreads), 0, st, slab, pitch, T, n_cols, D, packed, d_tab, tpitch);
    else
        hipLaunchKernelGGL(k_unwrap_ortho<false>, grid, dim3(kUnwrapThreads), 0, st, slab, pitch, T, n_cols, D, packed, d_tab, tpitch);
    return hipGetLastError();
}

}  // namespace ta
