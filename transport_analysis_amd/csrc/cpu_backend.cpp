// cpu_backend.cpp — the CPU backend behind the C-ABI ("a CPU backend behind the same
// symbols for parity / CI"; BASELINE.md section 4: "the build's own C++/OpenMP CPU backend on all host cores").
//
// STRICTLY OPT-IN: a context created with ta_ctx_create(TA_DEVICE_CPU, ...) computes here; every other context is
// a GPU context and fails loudly without a GPU.  Nothing in this file is reached from a GPU context, and nothing
// here uses oracle/ (test infrastructure) -- this is independent code: its own Stockham radix-4 transform, the
// windowed form, the difference-first Einstein-Helfand form.
//
// What it computes, per atom n of the staged (n_frames, n_atoms, dim) slabs (float32 or float64 elements, widened
// exactly), in float64:
//   FFT VACF      velocityautocorr.py:208-215 (+ tidynamics.acf): B[k, n] = sum_d sum_i v[i,n,d] v[i+k,n,d] / (T - k) by
//                 zero-padded transforms of length L = the power of two >= 2T (any pad >= 2T - 1 gives the same
//                 correlation); two columns ride one complex transform (z = x + i y: |Z|^2 transforms back to
//                 acf_x + acf_y), two atoms' power spectra one inverse (both real: untangled by the mirror bins);
//   windowed VACF velocityautocorr.py:217-238: the same sums, lag by lag, products then sum (k = 0 .. T - 1);
//   Helfand       viscosity.py:201-233: P = (m v) x, H[k, n] = scale / D / (T - k) sum_i sum_d (P[i] - P[i+k])^2,
//                 difference first, like the reference; H[0, n] = 0.
//   Einstein MSD  MDAnalysis.analysis.msd.EinsteinMSD: M[k, n] = 1 / (T - k) sum_i sum_d (x[i] - x[i+k])^2, M[0, n] = 0;
//                 fft = false difference first (the Helfand loop without masses and 1 / D), fft = true by the transforms
//                 of the FFT VACF on P = x - x[0] and S1 - 2 S2 (P's autocorrelation, prefix sums of sum_d P^2), as on
//                 the GPU (msd.hip).
//   Unwrap        MDAnalysis' NoJump in place (unwrap.hip's arithmetic): per atom, a walk along time carrying the integer
//                 image counts n(t) = n(t-1) + rint(f(t) - f(t-1)), f = x H^-1, and writing x - n H (rounded to the slab's
//                 element type: a float32 slab holds float32 positions, as NoJump writes them).
//   Conductivity  M[t, d] = sum_n q_n (x[t,n,d] - x[0,n,d]) (a frame per task, atoms in order); the collective MSD of M
//                 and the self term sum_n q_n^2 MSD_n as the Einstein MSD of a one-atom slab holding M and of the
//                 weighted slab q (x - x[0]).
// timeseries[k] = sum over atoms (the caller divides by n_atoms, as for the GPU path).  Atoms are processed in
// blocks of 8 by OpenMP threads; a block's lag sums are added in block order afterwards, so results do not depend on
// the number of threads.
#include <omp.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ta_hip.h"
#include "cpu_backend.hpp"
#include "kcurrent_math.hpp"
#include "chain_math.hpp"
#include "orient_math.hpp"
#include "bond_math.hpp"
#include "pair_math.hpp"
#include "shell_msd_math.hpp"
#include "shell_orient_math.hpp"
#include "unwrap_box.hpp"
#include "vanhove_distinct_math.hpp"
#include "vanhove_math.hpp"

namespace ta {
namespace cpu {
namespace {

constexpr int kBlock = 8;  // atoms per task: a block's by-particle values are written as rows of 8 doubles (one line)

// ---- power-of-two complex transform, split format, Stockham autosort, radix 4 (+ one radix-2 stage) -------------
// forward: X[k] = sum_n x[n] exp(-2 pi i n k / N)
struct Plan {
    int n = 0;
    // per radix-4 stage (sub-length m = n, n/4, ...): w1 = W_m^p, w2 = W_m^2p, w3 = W_m^3p, p < m / 4
    std::vector<double> tw;
    std::vector<size_t> off;  // offset of each stage's tables in tw
    explicit Plan(int n_) : n(n_) {
        const long double pi = 3.141592653589793238462643383279502884L;
        for (int m = n; m >= 4; m /= 4) {
            off.push_back(tw.size());
            const int q = m / 4;
            tw.resize(tw.size() + 6 * (size_t)q);
            double* t = tw.data() + off.back();
            for (int p = 0; p < q; ++p)
                for (int k = 1; k <= 3; ++k) {
                    const long double a = 2.0L * pi * (long double)(k * p) / (long double)m;
                    t[(2 * (k - 1)) * q + p] = (double)cosl(a);
                    t[(2 * (k - 1) + 1) * q + p] = (double)-sinl(a);
                }
        }
    }
};

// one radix-4 stage: x (sub-length m, stride s) -> y (sub-length m / 4, stride 4 s)
inline void stage4(int m, int s, const double* __restrict__ t, const double* __restrict__ xr, const double* __restrict__ xi,
                   double* __restrict__ yr, double* __restrict__ yi) {
    const int q4 = m / 4;
    const double *w1r = t, *w1i = t + q4, *w2r = t + 2 * q4, *w2i = t + 3 * q4, *w3r = t + 4 * q4, *w3i = t + 5 * q4;
    if (s == 1) {
        for (int p = 0; p < q4; ++p) {
            const double ar = xr[p], ai = xi[p], br = xr[p + q4], bi = xi[p + q4];
            const double cr = xr[p + 2 * q4], ci = xi[p + 2 * q4], dr = xr[p + 3 * q4], di = xi[p + 3 * q4];
            const double apcr = ar + cr, apci = ai + ci, amcr = ar - cr, amci = ai - ci;
            const double bpdr = br + dr, bpdi = bi + di;
            const double jr = -(bi - di), ji = br - dr;  // i (b - d)
            const double t1r = amcr - jr, t1i = amci - ji, t2r = apcr - bpdr, t2i = apci - bpdi;
            const double t3r = amcr + jr, t3i = amci + ji;
            yr[4 * p] = apcr + bpdr;
            yi[4 * p] = apci + bpdi;
            yr[4 * p + 1] = w1r[p] * t1r - w1i[p] * t1i;
            yi[4 * p + 1] = w1r[p] * t1i + w1i[p] * t1r;
            yr[4 * p + 2] = w2r[p] * t2r - w2i[p] * t2i;
            yi[4 * p + 2] = w2r[p] * t2i + w2i[p] * t2r;
            yr[4 * p + 3] = w3r[p] * t3r - w3i[p] * t3i;
            yi[4 * p + 3] = w3r[p] * t3i + w3i[p] * t3r;
        }
        return;
    }
    for (int p = 0; p < q4; ++p) {
        const double a1r = w1r[p], a1i = w1i[p], a2r = w2r[p], a2i = w2i[p], a3r = w3r[p], a3i = w3i[p];
        const double *x0r = xr + (size_t)s * p, *x0i = xi + (size_t)s * p;
        const double *x1r = x0r + (size_t)s * q4, *x1i = x0i + (size_t)s * q4;
        const double *x2r = x1r + (size_t)s * q4, *x2i = x1i + (size_t)s * q4;
        const double *x3r = x2r + (size_t)s * q4, *x3i = x2i + (size_t)s * q4;
        double *y0r = yr + (size_t)s * 4 * p, *y0i = yi + (size_t)s * 4 * p;
        double *y1r = y0r + s, *y1i = y0i + s, *y2r = y1r + s, *y2i = y1i + s, *y3r = y2r + s, *y3i = y2i + s;
#pragma omp simd
        for (int q = 0; q < s; ++q) {
            const double ar = x0r[q], ai = x0i[q], br = x1r[q], bi = x1i[q];
            const double cr = x2r[q], ci = x2i[q], dr = x3r[q], di = x3i[q];
            const double apcr = ar + cr, apci = ai + ci, amcr = ar - cr, amci = ai - ci;
            const double bpdr = br + dr, bpdi = bi + di;
            const double jr = -(bi - di), ji = br - dr;
            const double t1r = amcr - jr, t1i = amci - ji, t2r = apcr - bpdr, t2i = apci - bpdi;
            const double t3r = amcr + jr, t3i = amci + ji;
            y0r[q] = apcr + bpdr;
            y0i[q] = apci + bpdi;
            y1r[q] = a1r * t1r - a1i * t1i;
            y1i[q] = a1r * t1i + a1i * t1r;
            y2r[q] = a2r * t2r - a2i * t2i;
            y2i[q] = a2r * t2i + a2i * t2r;
            y3r[q] = a3r * t3r - a3i * t3i;
            y3i[q] = a3r * t3i + a3i * t3r;
        }
    }
}

// in: (ar, ai); scratch (br, bi); returns the pair of pointers that hold the result
struct Split {
    double *r, *i;
};
inline Split fft(const Plan& pl, double* ar, double* ai, double* br, double* bi) {
    int m = pl.n, s = 1;
    size_t st = 0;
    double *xr = ar, *xi = ai, *yr = br, *yi = bi;
    for (; m >= 4; m /= 4, s *= 4, ++st) {
        stage4(m, s, pl.tw.data() + pl.off[st], xr, xi, yr, yi);
        std::swap(xr, yr);
        std::swap(xi, yi);
    }
    if (m == 2) {  // the last radix-2 stage (log2 n odd): no twiddles
#pragma omp simd
        for (int q = 0; q < s; ++q) {
            const double a_r = xr[q], a_i = xi[q], b_r = xr[q + s], b_i = xi[q + s];
            yr[q] = a_r + b_r;
            yi[q] = a_i + b_i;
            yr[q + s] = a_r - b_r;
            yi[q + s] = a_i - b_i;
        }
        std::swap(xr, yr);
        std::swap(xi, yi);
    }
    return {xr, xi};
}

template <class E>
inline double elem(const void* slab, size_t idx) {
    return (double)static_cast<const E*>(slab)[idx];
}

struct Work {  // per-thread buffers
    std::vector<double> a, b, c, d, pr[2], cq[2], cols, prod, out;
};

// msd: the Einstein MSD of the slab instead of its autocorrelation (the columns shifted by their first frame, the
// prefix sums cq[h][t] = sum_{i<t} sum_d P[i]^2 of the atom, and the S1 - 2 S2 combination per lag)
template <class E>
int vacf_fft_t(const State& s, double* ts, double* bp, bool msd = false) {
    const int64_t T = s.T, A = s.A;
    const int D = s.D;
    int L = 2;
    while (L < 2 * T) L *= 2;
    const Plan plan(L);
    const int64_t n_blocks = (A + kBlock - 1) / kBlock;
    std::vector<double> part((size_t)n_blocks * T);
    const void* slab = s.slabs[0];
    bool oom = false;
#pragma omp parallel num_threads(s.threads)
    {
        Work w;
        try {
            for (auto* v : {&w.a, &w.b, &w.c, &w.d, &w.pr[0], &w.pr[1]}) v->assign((size_t)L, 0.0);
            if (msd)
                for (auto* v : {&w.cq[0], &w.cq[1]}) v->assign((size_t)T + 1, 0.0);
            w.out.assign((size_t)T * kBlock, 0.0);
        } catch (const std::bad_alloc&) {
#pragma omp atomic write
            oom = true;
        }
#pragma omp barrier
        if (!oom) {
#pragma omp for schedule(dynamic, 1)
            for (int64_t blk = 0; blk < n_blocks; ++blk) {
                const int64_t a0 = blk * kBlock, na = std::min<int64_t>(kBlock, A - a0);
                double* psum = part.data() + (size_t)blk * T;
                std::memset(psum, 0, sizeof(double) * T);
                for (int64_t j = 0; j < na; j += 2) {
                    const int n2 = j + 1 < na ? 2 : 1;
                    // the power spectra of one or two atoms
                    for (int h = 0; h < n2; ++h) {
                        const int64_t atom = a0 + j + h;
                        double* P = w.pr[h].data();
                        std::memset(P, 0, sizeof(double) * L);
                        if (msd) std::memset(w.cq[h].data(), 0, sizeof(double) * (T + 1));
                        for (int d0 = 0; d0 < D; d0 += 2) {
                            const bool two = d0 + 1 < D;
                            double *xr = w.a.data(), *xi = w.b.data();
                            for (int64_t t = 0; t < T; ++t) {
                                const size_t base = ((size_t)t * A + atom) * D + d0;
                                xr[t] = elem<E>(slab, base);
                                xi[t] = two ? elem<E>(slab, base + 1) : 0.0;
                            }
                            if (msd) {
                                const double x0 = xr[0], y0 = xi[0];
                                double* q = w.cq[h].data() + 1;
                                for (int64_t t = 0; t < T; ++t) {
                                    xr[t] -= x0;
                                    xi[t] -= y0;
                                    q[t] += xr[t] * xr[t] + xi[t] * xi[t];
                                }
                            }
                            std::memset(xr + T, 0, sizeof(double) * (L - T));
                            std::memset(xi + T, 0, sizeof(double) * (L - T));
                            const Split z = fft(plan, xr, xi, w.c.data(), w.d.data());
#pragma omp simd
                            for (int k = 0; k < L; ++k) P[k] += z.r[k] * z.r[k] + z.i[k] * z.i[k];
                        }
                        if (msd) {  // cq[h][t + 1] = Q[t] -> exclusive prefix sums C[0 .. T]
                            double* C = w.cq[h].data();
                            for (int64_t t = 1; t <= T; ++t) C[t] += C[t - 1];
                        }
                    }
                    // one transform of P_0 + i P_1 (both real: G[n] + conj G[L - n] = 2 F_0[n], the imaginary parts F_1)
                    double *gr = w.a.data(), *gi = w.b.data();
                    std::memcpy(gr, w.pr[0].data(), sizeof(double) * L);
                    if (n2 == 2) std::memcpy(gi, w.pr[1].data(), sizeof(double) * L);
                    else std::memset(gi, 0, sizeof(double) * L);
                    const Split g = fft(plan, gr, gi, w.c.data(), w.d.data());
                    for (int64_t n = 0; n < T; ++n) {
                        const int64_t mir = n == 0 ? 0 : L - n;
                        const double norm = (double)L * (double)(T - n);  // < 2^53: exact
                        double f[2] = {0.5 * (g.r[n] + g.r[mir]) / norm, 0.5 * (g.i[n] + g.i[mir]) / norm};
                        if (msd)
                            for (int h = 0; h < n2; ++h) {  // (C[T - n] + C[T] - C[n]) / (T - n) - 2 S2 / (T - n)
                                const double* C = w.cq[h].data();
                                f[h] = n == 0 ? 0.0 : (C[T - n] + (C[T] - C[n])) / (double)(T - n) - 2.0 * f[h];
                            }
                        w.out[(size_t)n * kBlock + j] = f[0];
                        if (n2 == 2) w.out[(size_t)n * kBlock + j + 1] = f[1];
                    }
                }
                for (int64_t n = 0; n < T; ++n) {
                    double sum = 0.0;
                    const double* row = w.out.data() + (size_t)n * kBlock;
                    for (int64_t j = 0; j < na; ++j) sum += row[j];
                    psum[n] = sum;
                    if (bp) std::memcpy(bp + (size_t)n * A + a0, row, sizeof(double) * na);
                }
            }
        }
    }
    if (oom) return TA_E_NOMEM;
    for (int64_t n = 0; n < T; ++n) {
        double sum = 0.0;
        for (int64_t blk = 0; blk < n_blocks; ++blk) sum += part[(size_t)blk * T + n];
        ts[n] = sum;
    }
    return TA_OK;
}

// windowed VACF (helfand == false), Einstein-Helfand (helfand == true) and the Einstein MSD (msd == true: slab 0 = the
// positions, differences as Helfand without masses and 1 / D) share the O(T^2) loop over lags
template <class E>
int direct_t(const State& s, bool helfand, const double* masses, double scale, double* ts, double* bp, bool msd = false) {
    const int64_t T = s.T, A = s.A;
    const int D = s.D;
    const int64_t n_blocks = (A + kBlock - 1) / kBlock;
    std::vector<double> part((size_t)n_blocks * T);
    const void *vel = s.slabs[0], *pos = helfand ? s.slabs[1] : nullptr;
    bool oom = false;
#pragma omp parallel num_threads(s.threads)
    {
        Work w;
        try {
            w.cols.assign((size_t)T * D, 0.0);
            w.out.assign((size_t)T * kBlock, 0.0);
        } catch (const std::bad_alloc&) {
#pragma omp atomic write
            oom = true;
        }
#pragma omp barrier
        if (!oom) {
#pragma omp for schedule(dynamic, 1)
            for (int64_t blk = 0; blk < n_blocks; ++blk) {
                const int64_t a0 = blk * kBlock, na = std::min<int64_t>(kBlock, A - a0);
                double* psum = part.data() + (size_t)blk * T;
                for (int64_t j = 0; j < na; ++j) {
                    const int64_t atom = a0 + j;
                    // the atom's columns, contiguous in time: c[d][t] (Helfand: P = (m v) x, the reference's order)
                    double* c = w.cols.data();
                    for (int d = 0; d < D; ++d)
                        for (int64_t t = 0; t < T; ++t) {
                            const size_t idx = ((size_t)t * A + atom) * D + d;
                            c[(size_t)d * T + t] = helfand ? (masses[atom] * elem<E>(vel, idx)) * elem<E>(pos, idx) : elem<E>(vel, idx);
                        }
                    for (int64_t k = 0; k < T; ++k) {
                        double acc = 0.0;
                        if (!((helfand || msd) && k == 0)) {
                            for (int d = 0; d < D; ++d) {
                                const double *p0 = c + (size_t)d * T, *p1 = p0 + k;
                                double sd = 0.0;
                                if (helfand || msd) {
#pragma omp simd reduction(+ : sd)
                                    for (int64_t i = 0; i < T - k; ++i) {
                                        const double df = p0[i] - p1[i];
                                        sd += df * df;
                                    }
                                } else {
#pragma omp simd reduction(+ : sd)
                                    for (int64_t i = 0; i < T - k; ++i) sd += p0[i] * p1[i];
                                }
                                acc += sd;
                            }
                            acc /= (double)(T - k);
                            if (helfand) acc = acc / (double)D * scale;  // mean over the columns (viscosity.py:222), then 1 / (2 kB V T)
                        }
                        w.out[(size_t)k * kBlock + j] = acc;
                    }
                }
                for (int64_t n = 0; n < T; ++n) {
                    double sum = 0.0;
                    const double* row = w.out.data() + (size_t)n * kBlock;
                    for (int64_t j = 0; j < na; ++j) sum += row[j];
                    psum[n] = sum;
                    if (bp) std::memcpy(bp + (size_t)n * A + a0, row, sizeof(double) * na);
                }
            }
        }
    }
    if (oom) return TA_E_NOMEM;
    for (int64_t n = 0; n < T; ++n) {
        double sum = 0.0;
        for (int64_t blk = 0; blk < n_blocks; ++blk) sum += part[(size_t)blk * T + n];
        ts[n] = sum;
    }
    return TA_OK;
}

}  // namespace

int hardware_threads() { return omp_get_max_threads(); }

// the benchmark generator of ta_stage_synth (layout.hip: synth_value; oracle/synth.py reproduces it): element (t, c) of the
// slab = value(seed, t n_cols_total + col_offset + c) -- integer arithmetic and ONE correctly rounded product: the same
// bits as on the GPU
static inline unsigned long long splitmix64(unsigned long long x) {
    unsigned long long z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline double synth_value(unsigned long long seed, unsigned long long idx) {
    const unsigned long long a = splitmix64(seed + 2 * idx), b = splitmix64(seed + 2 * idx + 1);
    long s = 0;
    for (int k = 0; k < 4; ++k) s += (long)((a >> (16 * k)) & 0xFFFF) + (long)((b >> (16 * k)) & 0xFFFF);
    return (double)(s - 262140) * 0x1.3988e1412ed76p-16;
}
void synth(const State& s, int slab, unsigned long long seed, int64_t col_offset, int64_t n_cols_total) {
    const int64_t T = s.T, n_cols = s.A * s.D;
    void* p = s.slabs[slab];
#pragma omp parallel for num_threads(s.threads) schedule(static)
    for (int64_t t = 0; t < T; ++t)
        for (int64_t c = 0; c < n_cols; ++c) {
            const double v = synth_value(seed, (unsigned long long)(t * n_cols_total + col_offset + c));
            if (s.dtype == TA_F32) static_cast<float*>(p)[(size_t)t * n_cols + c] = (float)v;
            else static_cast<double*>(p)[(size_t)t * n_cols + c] = v;
        }
}

bool supported() { return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma"); }

int vacf_fft(const State& s, double* ts, double* bp) {
    return s.dtype == TA_F32 ? vacf_fft_t<float>(s, ts, bp) : vacf_fft_t<double>(s, ts, bp);
}
int vacf_direct(const State& s, double* ts, double* bp) {
    return s.dtype == TA_F32 ? direct_t<float>(s, false, nullptr, 1.0, ts, bp) : direct_t<double>(s, false, nullptr, 1.0, ts, bp);
}
int helfand(const State& s, const double* masses, double scale, double* ts, double* bp) {
    return s.dtype == TA_F32 ? direct_t<float>(s, true, masses, scale, ts, bp) : direct_t<double>(s, true, masses, scale, ts, bp);
}
int msd(const State& s, bool fft, double* ts, double* bp) {
    if (fft) return s.dtype == TA_F32 ? vacf_fft_t<float>(s, ts, bp, true) : vacf_fft_t<double>(s, ts, bp, true);
    return s.dtype == TA_F32 ? direct_t<float>(s, false, nullptr, 1.0, ts, bp, true)
                             : direct_t<double>(s, false, nullptr, 1.0, ts, bp, true);
}

// moments (S, T, D) = sum_{n: species[n] = sp} w_n (x - x[0]) of slab 0, frame-parallel (species NULL: all atoms are species 0;
// w NULL: all 1), and with wslab the weighted shifted slab w_n (x - x[0]) in the slab's layout.  shift == false: the
// currents sum w_n x, nothing subtracted (x - 0.0 is x: one loop, and the same bits as before for the moments)
static void moments_of(const State& s, int S, const int32_t* species, const double* w, double* moments, double* wslab,
                       bool shift = true) {
    const int64_t T = s.T, A = s.A;
    const int D = s.D;
    const void* slab = s.slabs[0];
    const bool f32 = s.dtype == TA_F32;
#pragma omp parallel for num_threads(s.threads) schedule(static)
    for (int64_t t = 0; t < T; ++t) {
        double acc[8][3] = {};
        for (int64_t n = 0; n < A; ++n) {
            const double wn = w ? w[n] : 1.0;
            double* a = acc[species ? species[n] : 0];
            for (int d = 0; d < D; ++d) {
                const size_t i0 = (size_t)n * D + d, i = (size_t)t * A * D + i0;
                const double x = f32 ? elem<float>(slab, i) : elem<double>(slab, i);
                const double x0 = !shift ? 0.0 : f32 ? elem<float>(slab, i0) : elem<double>(slab, i0);
                const double v = wn * (x - x0);
                a[d] += v;
                if (wslab) wslab[i] = v;
            }
        }
        for (int sp = 0; sp < S; ++sp)
            for (int d = 0; d < D; ++d) moments[((size_t)sp * T + t) * D + d] = acc[sp][d];
    }
}

// a float64 (T, A, D) array as a slab of its own: what msd() reads for the weighted slab, the moment and the pseudo-particles
static State f64_slab(int threads, int64_t T, int64_t A, int D, double* data) {
    State v;
    v.T = T, v.A = A, v.D = D, v.dtype = TA_F64, v.threads = threads;
    v.slabs = {data};
    return v;
}

int conductivity(const State& s, bool fft, const double* q, double* moment, double* collective, double* self_lagsum) {
    std::vector<double> w;
    if (self_lagsum) {
        try {
            w.assign((size_t)s.T * s.A * s.D, 0.0);
        } catch (const std::bad_alloc&) {
            return TA_E_NOMEM;
        }
    }
    moments_of(s, 1, nullptr, q, moment, self_lagsum ? w.data() : nullptr);
    if (self_lagsum)
        if (int rc = msd(f64_slab(s.threads, s.T, s.A, s.D, w.data()), fft, self_lagsum, nullptr)) return rc;
    return collective ? msd(f64_slab(s.threads, s.T, 1, s.D, moment), fft, collective, nullptr) : TA_OK;
}

// C (T, S, S) of the (S, T, D) sums Q by polarisation: the S^2 pseudo-particles Q_i, Q_i + Q_j, Q_i - Q_j, ONE by-particle
// evaluation of them, C_ij = 1/4 (f(Q_i + Q_j) - f(Q_i - Q_j)).  acf false: f = the MSD (msd()), lag 0 exactly 0 (one frame:
// no evaluation); acf true: f = the autocorrelation (vacf_fft / vacf_direct), lag 0 kept.  A pair with an all-zero sum: 0.
static int cross_of(int threads, bool fft, bool acf, const double* sums, int S, int64_t T, int D, double* cross) {
    const int64_t P = (int64_t)S * S;
    std::vector<double> pm, bp, ts;
    try {
        pm.assign((size_t)T * P * D, 0.0);
        bp.assign((size_t)T * P, 0.0);
        ts.assign((size_t)T, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    bool nz[8] = {};
    for (int i = 0; i < S; ++i)
        for (int64_t k = 0; k < T * D && !nz[i]; ++k) nz[i] = sums[(size_t)i * T * D + k] != 0.0;
    for (int64_t t = 0; t < T; ++t)
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j)
                for (int d = 0; d < D; ++d) {
                    const double qi = sums[((size_t)i * T + t) * D + d], qj = sums[((size_t)j * T + t) * D + d];
                    pm[((size_t)t * P + i * S + j) * D + d] = i == j ? qi : i < j ? qi + qj : qi - qj;
                }
    const State v = f64_slab(threads, T, P, D, pm.data());
    int rc = TA_OK;
    if (acf) rc = fft ? vacf_fft(v, ts.data(), bp.data()) : vacf_direct(v, ts.data(), bp.data());
    else if (T >= 2) rc = msd(v, fft, ts.data(), bp.data());
    if (rc) return rc;
    for (int64_t k = 0; k < T; ++k)
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) {
                const int lo = i < j ? i : j, hi = i < j ? j : i;
                const double* row = bp.data() + (size_t)k * P;
                double c = 0.0;
                if ((acf || k > 0) && nz[i] && nz[j]) c = i == j ? row[i * S + i] : 0.25 * (row[lo * S + hi] - row[hi * S + lo]);
                cross[((size_t)k * S + i) * S + j] = c;
            }
    return TA_OK;
}
int onsager_cross(int threads, bool fft, const double* moments, int S, int64_t T, int D, double* cross) {
    return cross_of(threads, fft, false, moments, S, T, D, cross);
}
int current_cross(int threads, bool fft, const double* currents, int S, int64_t T, int D, double* cross) {
    return cross_of(threads, fft, true, currents, S, T, D, cross);
}

int onsager(const State& s, bool fft, int S, const int32_t* species, const double* w, double* moments, double* cross) {
    moments_of(s, S, species, w, moments, nullptr);
    return cross ? onsager_cross(s.threads, fft, moments, S, s.T, s.D, cross) : TA_OK;
}
int current(const State& s, bool fft, int S, const int32_t* species, const double* w, double* currents, double* cross) {
    moments_of(s, S, species, w, currents, nullptr, false);
    return cross ? current_cross(s.threads, fft, currents, S, s.T, s.D, cross) : TA_OK;
}

int species_self(const State& s, bool msd_quantity, bool fft, int S, const int32_t* species, const double* w, double* self,
                 int64_t* counts) {
    const int64_t T = s.T, A = s.A;
    const int D = s.D;
    const void* slab = s.slabs[0];
    const bool f32 = s.dtype == TA_F32;
    for (int sp = 0; sp < S; ++sp) {
        std::vector<int64_t> atoms;
        std::vector<double> ws;
        try {
            for (int64_t n = 0; n < A; ++n)
                if (species[n] == sp) atoms.push_back(n);
            ws.assign((size_t)T * atoms.size() * D, 0.0);
        } catch (const std::bad_alloc&) {
            return TA_E_NOMEM;
        }
        const int64_t N = (int64_t)atoms.size();
        if (counts) counts[sp] = N;
        double* out = self + (size_t)sp * T;
        std::fill(out, out + T, 0.0);
        if (N == 0) continue;
#pragma omp parallel for num_threads(s.threads) schedule(static)
        for (int64_t t = 0; t < T; ++t)
            for (int64_t r = 0; r < N; ++r) {
                const int64_t n = atoms[r];
                const double wn = w ? w[n] : 1.0;
                for (int d = 0; d < D; ++d) {
                    const size_t i0 = (size_t)n * D + d, i = (size_t)t * A * D + i0;
                    const double x = f32 ? elem<float>(slab, i) : elem<double>(slab, i);
                    const double x0 = !msd_quantity ? 0.0 : f32 ? elem<float>(slab, i0) : elem<double>(slab, i0);
                    ws[((size_t)t * N + r) * D + d] = wn * (x - x0);
                }
            }
        const State v = f64_slab(s.threads, T, N, D, ws.data());
        if (int rc = msd_quantity ? msd(v, fft, out, nullptr) : fft ? vacf_fft(v, out, nullptr) : vacf_direct(v, out, nullptr))
            return rc;
    }
    return TA_OK;
}

int scatter_collective(int threads, bool fft, const double* density, int K, int64_t T, double* coll) {
    std::vector<double> pm, bp, ts;
    try {
        pm.assign((size_t)T * K * 2, 0.0);
        bp.assign((size_t)T * K, 0.0);
        ts.assign((size_t)T, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    for (int64_t t = 0; t < T; ++t)
        for (int j = 0; j < K; ++j)
            for (int h = 0; h < 2; ++h) pm[((size_t)t * K + j) * 2 + h] = density[((size_t)j * T + t) * 2 + h];
    const State v = f64_slab(threads, T, K, 2, pm.data());
    if (int rc = fft ? vacf_fft(v, ts.data(), bp.data()) : vacf_direct(v, ts.data(), bp.data())) return rc;
    for (int j = 0; j < K; ++j)
        for (int64_t t = 0; t < T; ++t) coll[(size_t)j * T + t] = bp[(size_t)t * K + j];
    return TA_OK;
}

int scatter(const State& s, bool fft, int K, const double* kvecs, double* self, double* density, double* coll) {
    const int64_t T = s.T, A = s.A;
    const int D = s.D;
    const void* slab = s.slabs[0];
    const bool f32 = s.dtype == TA_F32;
    std::vector<double> z, rho;
    try {
        z.assign((size_t)T * A * 2, 0.0);
        if (!density && coll) rho.assign((size_t)K * T * 2, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    double* dens = density ? density : rho.data();
    for (int j = 0; j < K; ++j) {
        double q[3] = {0.0, 0.0, 0.0};
        for (int d = 0; d < D; ++d) q[d] = kvecs[(size_t)j * D + d] / 6.283185307179586476925;
#pragma omp parallel for num_threads(s.threads) schedule(static)
        for (int64_t t = 0; t < T; ++t) {
            double sc = 0.0, ss = 0.0;
            for (int64_t n = 0; n < A; ++n) {
                const size_t i = ((size_t)t * A + n) * D;
                double u = q[0] * (f32 ? elem<float>(slab, i) : elem<double>(slab, i));
                for (int d = 1; d < D; ++d) u = std::fma(q[d], f32 ? elem<float>(slab, i + d) : elem<double>(slab, i + d), u);
                const double a = 6.283185307179586476925 * (u - std::nearbyint(u));
                const double c = std::cos(a), sn = std::sin(a);
                z[((size_t)t * A + n) * 2] = c, z[((size_t)t * A + n) * 2 + 1] = sn;
                sc += c, ss += sn;
            }
            if (density || coll) dens[((size_t)j * T + t) * 2] = sc, dens[((size_t)j * T + t) * 2 + 1] = ss;
        }
        if (self) {
            const State v = f64_slab(s.threads, T, A, 2, z.data());
            double* out = self + (size_t)j * T;
            if (int rc = fft ? vacf_fft(v, out, nullptr) : vacf_direct(v, out, nullptr)) return rc;
        }
    }
    return coll ? scatter_collective(s.threads, fft, dens, K, T, coll) : TA_OK;
}

template <class E, int MODE, bool PERIODIC>
static void orient_frames(const State& s, int64_t N, const int32_t* index, const double* box, int64_t tpitch, const double* w,
                          double* u_out, double* q_out, double* total) {
    const int64_t T = s.T, A = s.A;
    const void* slab = s.slabs[0];
    constexpr int K = MODE == ORIENT_BOND ? 2 : 3;
#pragma omp parallel for num_threads(s.threads) schedule(static)
    for (int64_t t = 0; t < T; ++t) {
        OrientBox bx{};
        if (PERIODIC) {
            const double* b = box + (tpitch == 1 ? 0 : t);
            bx = OrientBox{b[0], b[tpitch], b[2 * tpitch], b[3 * tpitch], b[4 * tpitch], b[5 * tpitch], b[6 * tpitch], b[7 * tpitch],
                           b[8 * tpitch]};
        }
        double m[3] = {0.0, 0.0, 0.0};
        for (int64_t n = 0; n < N; ++n) {
            double x[3][3] = {};
            for (int j = 0; j < K; ++j)
                for (int d = 0; d < 3; ++d) x[j][d] = elem<E>(slab, ((size_t)t * A + (size_t)index[n * K + j]) * 3 + d);
            double db[3], dc[3] = {0.0, 0.0, 0.0}, v[3], u[3];
            orient_diff<PERIODIC>(x[0], x[1], bx, db);
            if (MODE != ORIENT_BOND) orient_diff<PERIODIC>(x[0], x[2], bx, dc);
            orient_combine<MODE>(db, dc, v);
            orient_unit(v, u);
            if (u_out)
                for (int d = 0; d < 3; ++d) u_out[((size_t)t * N + n) * 3 + d] = u[d];
            if (q_out) orient_q(u, *reinterpret_cast<double(*)[6]>(q_out + ((size_t)t * N + n) * 6));
            if (total) {
                const double wn = w ? w[n] : 1.0;
                for (int d = 0; d < 3; ++d) m[d] += wn * u[d];
            }
        }
        if (total)
            for (int d = 0; d < 3; ++d) total[(size_t)t * 3 + d] = m[d];
    }
}

template <class E, int MODE>
static void orient_frames_box(const State& s, int64_t N, const int32_t* index, const double* box, int64_t tpitch, const double* w,
                              double* u_out, double* q_out, double* total) {
    if (box) orient_frames<E, MODE, true>(s, N, index, box, tpitch, w, u_out, q_out, total);
    else orient_frames<E, MODE, false>(s, N, index, box, tpitch, w, u_out, q_out, total);
}
template <class E>
static void orient_frames_mode(int mode, const State& s, int64_t N, const int32_t* index, const double* box, int64_t tpitch,
                               const double* w, double* u_out, double* q_out, double* total) {
    if (mode == ORIENT_BOND) orient_frames_box<E, ORIENT_BOND>(s, N, index, box, tpitch, w, u_out, q_out, total);
    else if (mode == ORIENT_BISECTOR) orient_frames_box<E, ORIENT_BISECTOR>(s, N, index, box, tpitch, w, u_out, q_out, total);
    else orient_frames_box<E, ORIENT_NORMAL>(s, N, index, box, tpitch, w, u_out, q_out, total);
}

int orient(const State& s, bool fft, int mode, int64_t N, const int32_t* index, const double* box, int64_t tpitch, const double* w,
           double* c1, double* c2, double* total, double* coll) {
    const int64_t T = s.T;
    std::vector<double> u, q, own;
    try {
        if (c1) u.assign((size_t)T * N * 3, 0.0);
        if (c2) q.assign((size_t)T * N * 6, 0.0);
        if (!total && coll) own.assign((size_t)T * 3, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    double* tot = total ? total : coll ? own.data() : nullptr;
    double* up = c1 ? u.data() : nullptr;
    double* qp = c2 ? q.data() : nullptr;
    if (s.dtype == TA_F32) orient_frames_mode<float>(mode, s, N, index, box, tpitch, w, up, qp, tot);
    else orient_frames_mode<double>(mode, s, N, index, box, tpitch, w, up, qp, tot);
    auto acf = [&](int64_t A, double* data, double* out) {
        const State v = f64_slab(s.threads, T, A, 3, data);
        return fft ? vacf_fft(v, out, nullptr) : vacf_direct(v, out, nullptr);
    };
    if (c1)
        if (int rc = acf(N, up, c1)) return rc;
    if (c2)  // the (T, N, 6) array is a slab of 2 N pseudo-atoms with dim 3
        if (int rc = acf(2 * N, qp, c2)) return rc;
    if (coll) {
        std::vector<double> m(tot, tot + (size_t)T * 3);  // (the evaluation may not write to the caller's total)
        if (int rc = acf(1, m.data(), coll)) return rc;
    }
    return TA_OK;
}

// y (Q, T, C, 3): functional q of chain c in frame t, by chain_math.hpp's sequence in bead order
template <class E, bool PERIODIC>
static void chain_frames(const State& s, int64_t C, int64_t N, const int32_t* members, int Q, const double* coeff, const double* box,
                         int64_t tpitch, double* y) {
    const int64_t T = s.T, A = s.A;
    const void* slab = s.slabs[0];
#pragma omp parallel for num_threads(s.threads) schedule(static)
    for (int64_t c = 0; c < C; ++c) {
        const int32_t* row = members + c * N;
        std::vector<double> acc((size_t)Q * 3);
        for (int64_t t = 0; t < T; ++t) {
            OrientBox bx{};
            if (PERIODIC) {
                const double* b = box + (tpitch == 1 ? 0 : t);
                bx = OrientBox{b[0], b[tpitch], b[2 * tpitch], b[3 * tpitch], b[4 * tpitch], b[5 * tpitch], b[6 * tpitch], b[7 * tpitch],
                               b[8 * tpitch]};
            }
            std::fill(acc.begin(), acc.end(), 0.0);
            double prev[3], cur[3], sum[3] = {0.0, 0.0, 0.0};
            for (int d = 0; d < 3; ++d) prev[d] = elem<E>(slab, ((size_t)t * A + (size_t)row[0]) * 3 + d);
            for (int64_t n = 1; n < N; ++n) {
                for (int d = 0; d < 3; ++d) cur[d] = elem<E>(slab, ((size_t)t * A + (size_t)row[n]) * 3 + d);
                chain_step<PERIODIC>(prev, cur, bx, sum);
                for (int q = 0; q < Q; ++q) chain_term(coeff[(size_t)q * N + n], sum, *reinterpret_cast<double(*)[3]>(&acc[(size_t)q * 3]));
                for (int d = 0; d < 3; ++d) prev[d] = cur[d];
            }
            for (int q = 0; q < Q; ++q)
                for (int d = 0; d < 3; ++d) y[(((size_t)q * T + t) * C + c) * 3 + d] = acc[(size_t)q * 3 + d];
        }
    }
}

int chain_modes(const State& s, bool fft, int64_t C, int64_t N, const int32_t* members, int Q, const double* coeff, const double* box,
                int64_t tpitch, double* acf) {
    const int64_t T = s.T;
    std::vector<double> y;
    try {
        y.assign((size_t)Q * T * C * 3, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    if (s.dtype == TA_F32) {
        if (box) chain_frames<float, true>(s, C, N, members, Q, coeff, box, tpitch, y.data());
        else chain_frames<float, false>(s, C, N, members, Q, coeff, box, tpitch, y.data());
    } else {
        if (box) chain_frames<double, true>(s, C, N, members, Q, coeff, box, tpitch, y.data());
        else chain_frames<double, false>(s, C, N, members, Q, coeff, box, tpitch, y.data());
    }
    for (int q = 0; q < Q; ++q) {
        const State v = f64_slab(s.threads, T, C, 3, y.data() + (size_t)q * T * C * 3);
        double* out = acf + (size_t)q * T;
        if (int rc = fft ? vacf_fft(v, out, nullptr) : vacf_direct(v, out, nullptr)) return rc;
    }
    return TA_OK;
}

int kcurrent_correlate(int threads, bool fft, const double* current, int K, const double* kvecs, int64_t T, int D, double* lon,
                       double* trans) {
    const int S = kcur_series(D);
    const int64_t P = (int64_t)K * S;
    std::vector<double> pm, bp, ts;
    try {
        pm.assign((size_t)T * P * 2, 0.0);
        bp.assign((size_t)T * P, 0.0);
        ts.assign((size_t)T, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    for (int j = 0; j < K; ++j) {
        double kh[3] = {0.0, 0.0, 0.0}, out[8];
        kcur_khat(D, kvecs + (size_t)j * D, kh);
        for (int64_t t = 0; t < T; ++t) {
            kcur_project(D, kh, current + ((size_t)j * T + t) * D * 2, out);
            for (int c = 0; c < 2 * S; ++c) pm[((size_t)t * P + (size_t)j * S) * 2 + c] = out[c];
        }
    }
    const State v = f64_slab(threads, T, P, 2, pm.data());
    if (int rc = fft ? vacf_fft(v, ts.data(), bp.data()) : vacf_direct(v, ts.data(), bp.data())) return rc;
    for (int j = 0; j < K; ++j)
        for (int64_t t = 0; t < T; ++t) {
            double l, tr;
            kcur_finish(D, bp.data() + (size_t)t * P + (size_t)j * S, &l, &tr);
            if (lon) lon[(size_t)j * T + t] = l;
            if (trans) trans[(size_t)j * T + t] = tr;
        }
    return TA_OK;
}

int kcurrent(const State& s, bool fft, int K, const double* kvecs, const double* w, double* current, double* lon, double* trans) {
    const int64_t T = s.T, A = s.A;
    const int D = s.D;
    const void *vel = s.slabs[0], *pos = s.slabs[1];
    const bool f32 = s.dtype == TA_F32;
    std::vector<double> own;
    if (!current) {
        try {
            own.assign((size_t)K * T * D * 2, 0.0);
        } catch (const std::bad_alloc&) {
            return TA_E_NOMEM;
        }
    }
    double* cur = current ? current : own.data();
    for (int j = 0; j < K; ++j) {
        double q[3] = {0.0, 0.0, 0.0};
        for (int d = 0; d < D; ++d) q[d] = kvecs[(size_t)j * D + d] / 6.283185307179586476925;
#pragma omp parallel for num_threads(s.threads) schedule(static)
        for (int64_t t = 0; t < T; ++t) {
            double re[3] = {0.0, 0.0, 0.0}, im[3] = {0.0, 0.0, 0.0};
            for (int64_t n = 0; n < A; ++n) {
                const size_t i = ((size_t)t * A + n) * D;
                double u = q[0] * (f32 ? elem<float>(pos, i) : elem<double>(pos, i));
                for (int d = 1; d < D; ++d) u = std::fma(q[d], f32 ? elem<float>(pos, i + d) : elem<double>(pos, i + d), u);
                const double a = 6.283185307179586476925 * (u - std::nearbyint(u));
                const double c = std::cos(a), sn = std::sin(a);
                const double wn = w ? w[n] : 1.0;
                for (int d = 0; d < D; ++d) {
                    const double wv = wn * (f32 ? elem<float>(vel, i + d) : elem<double>(vel, i + d));
                    re[d] = std::fma(wv, c, re[d]);
                    im[d] = std::fma(wv, sn, im[d]);
                }
            }
            for (int d = 0; d < D; ++d) {
                cur[(((size_t)j * T + t) * D + d) * 2] = re[d];
                cur[(((size_t)j * T + t) * D + d) * 2 + 1] = im[d];
            }
        }
    }
    return lon || trans ? kcurrent_correlate(s.threads, fft, cur, K, kvecs, T, D, lon, trans) : TA_OK;
}

int partial_cross(int threads, bool fft, const double* density, int K, int S, int64_t T, double* cross) {
    // a complex density is a species sum with dim 2: wavevector j's (S, T, 2) block is what current_cross takes
    for (int j = 0; j < K; ++j)
        if (int rc = current_cross(threads, fft, density + (size_t)j * S * T * 2, S, T, 2, cross + (size_t)j * T * S * S)) return rc;
    return TA_OK;
}

int partial_density(const State& s, bool fft, int K, const double* kvecs, int S, const int32_t* species, const double* w,
                    double* density, double* cross) {
    const int64_t T = s.T, A = s.A;
    const int D = s.D;
    const void* pos = s.slabs[0];
    const bool f32 = s.dtype == TA_F32;
    for (int j = 0; j < K; ++j) {
        double q[3] = {0.0, 0.0, 0.0};
        for (int d = 0; d < D; ++d) q[d] = kvecs[(size_t)j * D + d] / 6.283185307179586476925;
#pragma omp parallel for num_threads(s.threads) schedule(static)
        for (int64_t t = 0; t < T; ++t) {
            double re[8] = {}, im[8] = {};
            for (int64_t n = 0; n < A; ++n) {
                const size_t i = ((size_t)t * A + n) * D;
                double u = q[0] * (f32 ? elem<float>(pos, i) : elem<double>(pos, i));
                for (int d = 1; d < D; ++d) u = std::fma(q[d], f32 ? elem<float>(pos, i + d) : elem<double>(pos, i + d), u);
                const double a = 6.283185307179586476925 * (u - std::nearbyint(u));
                const double wn = w ? w[n] : 1.0;
                const int lab = species[n];
                re[lab] = std::fma(wn, std::cos(a), re[lab]);
                im[lab] = std::fma(wn, std::sin(a), im[lab]);
            }
            for (int a = 0; a < S; ++a) {
                density[(((size_t)j * S + a) * T + t) * 2] = re[a];
                density[(((size_t)j * S + a) * T + t) * 2 + 1] = im[a];
            }
        }
    }
    return cross ? partial_cross(s.threads, fft, density, K, S, T, cross) : TA_OK;
}

// Atoms in blocks of kVhBlock: OpenMP threads take atoms of a block, each with an int64 histogram of its own and every
// atom's moments in a slot of its own; after a block the moments are added in atom order, after the last one the threads'
// histograms: neither depends on the number of threads
constexpr int64_t kVhBlock = 1024;

template <class E, int D>
int vanhove_t(const State& s, int L, const int64_t* lags, int B, double dr, int64_t* counts, double* moments) {
    const int64_t T = s.T, A = s.A;
    const E* x = static_cast<const E*>(s.slabs[0]);
    const int nth = s.threads > 0 ? s.threads : 1;
    const size_t nb = (size_t)B + 1, nh = (size_t)L * nb;
    std::vector<double> e, mom;
    std::vector<int64_t> hist;
    try {
        e.assign(nb, 0.0);
        if (counts) hist.assign((size_t)nth * nh, 0);
        if (moments) mom.assign((size_t)kVhBlock * L * 2, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    vh_edges(B, dr, e.data());
    const float inv = vh_inv_dr(dr);
    if (moments) std::fill(moments, moments + 2 * (size_t)L, 0.0);
    for (int64_t n0 = 0; n0 < A; n0 += kVhBlock) {
        const int64_t n1 = std::min(A, n0 + kVhBlock);
#pragma omp parallel for num_threads(nth) schedule(static)
        for (int64_t n = n0; n < n1; ++n) {
            int64_t* h = counts ? hist.data() + (size_t)omp_get_thread_num() * nh : nullptr;
            for (int l = 0; l < L; ++l) {
                const int64_t tau = lags[l];
                double s2 = 0.0, s4 = 0.0;
                for (int64_t t = 0; t + tau < T; ++t) {
                    double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
                    for (int d = 0; d < D; ++d) {
                        a[d] = (double)x[((size_t)t * A + n) * D + d];
                        b[d] = (double)x[((size_t)(t + tau) * A + n) * D + d];
                    }
                    const double r2 = vh_r2<D>(a, b);
                    s2 += r2;
                    s4 = std::fma(r2, r2, s4);
                    if (h) ++h[l * nb + vh_bin(r2, e.data(), B, inv)];
                }
                if (moments) mom[((size_t)(n - n0) * L + l) * 2] = s2, mom[((size_t)(n - n0) * L + l) * 2 + 1] = s4;
            }
        }
        if (moments)
            for (int64_t n = n0; n < n1; ++n)
                for (size_t i = 0; i < 2 * (size_t)L; ++i) moments[i] += mom[(size_t)(n - n0) * L * 2 + i];
    }
    if (counts) {
        std::fill(counts, counts + nh, (int64_t)0);
        for (int th = 0; th < nth; ++th)
            for (size_t i = 0; i < nh; ++i) counts[i] += hist[(size_t)th * nh + i];
    }
    return TA_OK;
}

template <class E>
int vanhove_e(const State& s, int L, const int64_t* lags, int B, double dr, int64_t* counts, double* moments) {
    if (s.D == 1) return vanhove_t<E, 1>(s, L, lags, B, dr, counts, moments);
    if (s.D == 2) return vanhove_t<E, 2>(s, L, lags, B, dr, counts, moments);
    return vanhove_t<E, 3>(s, L, lags, B, dr, counts, moments);
}

int vanhove(const State& s, int L, const int64_t* lags, int B, double dr, int64_t* counts, double* moments) {
    return s.dtype == TA_F32 ? vanhove_e<float>(s, L, lags, B, dr, counts, moments) : vanhove_e<double>(s, L, lags, B, dr, counts, moments);
}

// The self-overlap per origin.  The host slab is frame-major: the atoms of frames t0 and t0 + tau are two contiguous runs,
// so a thread that owns (l, t0) streams both and writes its C counts -- no two threads share an element of q.
template <class E, int D>
int overlap_t(const State& s, int L, const int64_t* lags, int C, const double* cutoffs, int64_t* q) {
    const int64_t T = s.T, A = s.A;
    const E* x = static_cast<const E*>(s.slabs[0]);
    const int nth = s.threads > 0 ? s.threads : 1;
    double a2[TA_OVERLAP_MAX_CUTOFFS];
    vh_cutoffs2(C, cutoffs, a2);
    std::fill(q, q + (size_t)C * L * T, (int64_t)0);
#pragma omp parallel for num_threads(nth) schedule(static) collapse(2)
    for (int l = 0; l < L; ++l) {
        for (int64_t t = 0; t < T; ++t) {
            const int64_t tau = lags[l];
            if (t + tau >= T) continue;
            int64_t cnt[TA_OVERLAP_MAX_CUTOFFS] = {0, 0, 0, 0};
            const E* x0 = x + (size_t)t * A * D;
            const E* x1 = x + (size_t)(t + tau) * A * D;
            for (int64_t n = 0; n < A; ++n) {
                double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
                for (int d = 0; d < D; ++d) {
                    a[d] = (double)x0[n * D + d];
                    b[d] = (double)x1[n * D + d];
                }
                const double r2 = vh_r2<D>(a, b);
                for (int c = 0; c < C; ++c) cnt[c] += r2 < a2[c] ? 1 : 0;
            }
            for (int c = 0; c < C; ++c) q[((size_t)c * L + l) * T + t] = cnt[c];
        }
    }
    return TA_OK;
}

template <class E>
int overlap_e(const State& s, int L, const int64_t* lags, int C, const double* cutoffs, int64_t* q) {
    if (s.D == 1) return overlap_t<E, 1>(s, L, lags, C, cutoffs, q);
    if (s.D == 2) return overlap_t<E, 2>(s, L, lags, C, cutoffs, q);
    return overlap_t<E, 3>(s, L, lags, C, cutoffs, q);
}

int overlap(const State& s, int L, const int64_t* lags, int C, const double* cutoffs, int64_t* q) {
    return s.dtype == TA_F32 ? overlap_e<float>(s, L, lags, C, cutoffs, q) : overlap_e<double>(s, L, lags, C, cutoffs, q);
}

// (cos, sin)(pi y), |y| <= 1, as sincospi gives it on the device to within an ulp: the half turns are folded away exactly
// first (|y| = n / 2 + f, |f| <= 1 / 4), so the quarter turns come out as exact 0 and +-1
inline void od_sincospi(double y, double* sn, double* cs) {
    const double ay = std::fabs(y);
    const double n = std::nearbyint(2.0 * ay);  // 0, 1 or 2
    const double f = 3.141592653589793238463 * (ay - 0.5 * n);
    const double sf = std::sin(f), cf = std::cos(f);
    double s_, c_;
    if (n == 0.0) s_ = sf, c_ = cf;
    else if (n == 1.0) s_ = cf, c_ = -sf;
    else s_ = -sf, c_ = -cf;
    *sn = y < 0.0 ? -s_ : s_;
    *cs = c_;
}

// The overlap field's density per origin.  As overlap_t: a thread that owns (l, t0) streams the two frames' atoms in atom
// order and writes its K C sums -- no two threads share an element of w, and nothing depends on the thread count.  The
// phase is phase_math.hpp's expression (q = k / 2 pi, u by product-then-fma, r = u - rint(u), sincospi(2 r)) of the ORIGIN
// frame, r2 and a2 are vanhove_math.hpp's, the update is a select.  Wavevectors in blocks of kOdBlock keep the sums on the stack.
constexpr int kOdBlock = 16;

template <class E, int D>
int overlap_density_t(const State& s, int K, const double* kvecs, int L, const int64_t* lags, int C, const double* cutoffs,
                      double* w) {
    const int64_t T = s.T, A = s.A;
    const E* x = static_cast<const E*>(s.slabs[0]);
    const int nth = s.threads > 0 ? s.threads : 1;
    double a2[TA_OVERLAP_MAX_CUTOFFS];
    vh_cutoffs2(C, cutoffs, a2);
    std::vector<double> q;
    try {
        q.assign((size_t)K * 3, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    for (int j = 0; j < K; ++j)
        for (int d = 0; d < D; ++d) q[(size_t)j * 3 + d] = kvecs[(size_t)j * D + d] / 6.283185307179586476925;
    std::fill(w, w + 2 * (size_t)K * C * L * T, 0.0);
    for (int j0 = 0; j0 < K; j0 += kOdBlock) {
        const int kb = std::min(kOdBlock, K - j0);
#pragma omp parallel for num_threads(nth) schedule(static) collapse(2)
        for (int l = 0; l < L; ++l) {
            for (int64_t t = 0; t < T; ++t) {
                const int64_t tau = lags[l];
                if (t + tau >= T) continue;
                double re[kOdBlock][TA_OVERLAP_MAX_CUTOFFS] = {}, im[kOdBlock][TA_OVERLAP_MAX_CUTOFFS] = {};
                const E* x0 = x + (size_t)t * A * D;
                const E* x1 = x + (size_t)(t + tau) * A * D;
                for (int64_t n = 0; n < A; ++n) {
                    double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
                    for (int d = 0; d < D; ++d) {
                        a[d] = (double)x0[n * D + d];
                        b[d] = (double)x1[n * D + d];
                    }
                    const double r2 = vh_r2<D>(a, b);
                    if (!(r2 < a2[C - 1])) continue;  // (the cutoffs increase: outside the largest is outside all)
                    for (int jl = 0; jl < kb; ++jl) {
                        const double* qj = q.data() + (size_t)(j0 + jl) * 3;
                        double u = qj[0] * a[0];
                        if (D > 1) u = std::fma(qj[1], a[1], u);
                        if (D > 2) u = std::fma(qj[2], a[2], u);
                        const double r = u - std::nearbyint(u);
                        double sn, cs;
                        od_sincospi(2.0 * r, &sn, &cs);
                        for (int c = 0; c < C; ++c) {
                            const bool inside = r2 < a2[c];
                            re[jl][c] = inside ? re[jl][c] + cs : re[jl][c];
                            im[jl][c] = inside ? im[jl][c] + sn : im[jl][c];
                        }
                    }
                }
                for (int jl = 0; jl < kb; ++jl)
                    for (int c = 0; c < C; ++c) {
                        double* o = w + ((((size_t)(j0 + jl) * C + c) * L + l) * T + t) * 2;
                        o[0] = re[jl][c], o[1] = im[jl][c];
                    }
            }
        }
    }
    return TA_OK;
}

template <class E>
int overlap_density_e(const State& s, int K, const double* kvecs, int L, const int64_t* lags, int C, const double* cutoffs, double* w) {
    if (s.D == 1) return overlap_density_t<E, 1>(s, K, kvecs, L, lags, C, cutoffs, w);
    if (s.D == 2) return overlap_density_t<E, 2>(s, K, kvecs, L, lags, C, cutoffs, w);
    return overlap_density_t<E, 3>(s, K, kvecs, L, lags, C, cutoffs, w);
}

int overlap_density(const State& s, int K, const double* kvecs, int L, const int64_t* lags, int C, const double* cutoffs, double* w) {
    return s.dtype == TA_F32 ? overlap_density_e<float>(s, K, kvecs, L, lags, C, cutoffs, w)
                             : overlap_density_e<double>(s, K, kvecs, L, lags, C, cutoffs, w);
}

// fn(E(), D, PERIODIC) as template arguments for the staged element type, dim and box
#define TA_PAIR_DISPATCH(fn, ...)                                                                                  \
    do {                                                                                                           \
        const bool f32 = s.dtype == TA_F32;                                                                        \
        if (hm) {                                                                                                  \
            if (s.D == 1) return f32 ? fn<float, 1, true>(__VA_ARGS__) : fn<double, 1, true>(__VA_ARGS__);         \
            if (s.D == 2) return f32 ? fn<float, 2, true>(__VA_ARGS__) : fn<double, 2, true>(__VA_ARGS__);         \
            return f32 ? fn<float, 3, true>(__VA_ARGS__) : fn<double, 3, true>(__VA_ARGS__);                       \
        }                                                                                                          \
        if (s.D == 1) return f32 ? fn<float, 1, false>(__VA_ARGS__) : fn<double, 1, false>(__VA_ARGS__);           \
        if (s.D == 2) return f32 ? fn<float, 2, false>(__VA_ARGS__) : fn<double, 2, false>(__VA_ARGS__);           \
        return f32 ? fn<float, 3, false>(__VA_ARGS__) : fn<double, 3, false>(__VA_ARGS__);                         \
    } while (0)

// the box of frame t: H[3], M[3] of the staged columns (ones without a box and on the axes past D)
template <int D, bool PERIODIC>
inline void frame_box(const double* hm, bool per_frame, int64_t t, double (&H)[3], double (&M)[3]) {
    for (int d = 0; d < 3; ++d) H[d] = 1.0, M[d] = 1.0;
    if (PERIODIC) {
        const double* box = hm + (per_frame ? t * 6 : 0);
        for (int d = 0; d < D; ++d) H[d] = box[d], M[d] = box[3 + d];
    }
}

// The distinct van Hove histogram: OpenMP threads take (origin, tile of kVhdCpuTile a-items) units, each thread with an int64
// histogram of its own; the threads' histograms are added at the end.  Integer adds only: nothing depends on the number of
// threads or on which thread took which unit.
constexpr int64_t kVhdCpuTile = 64;

template <class E, int D, bool PERIODIC>
int vanhove_distinct_t(const State& s, int L, const int64_t* lags, int64_t stride, int64_t n_a, const int32_t* ida, int64_t n_b,
                       const int32_t* idb, const double* hm, bool per_frame, int B, double dr, int64_t* counts) {
    const int64_t T = s.T, A = s.A;
    const E* x = static_cast<const E*>(s.slabs[0]);
    const int nth = s.threads > 0 ? s.threads : 1;
    const size_t nb = (size_t)B + 1, nh = (size_t)L * nb;
    std::vector<double> e;
    std::vector<int64_t> hist;
    try {
        e.assign(nb, 0.0);
        hist.assign((size_t)nth * nh, 0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    vh_edges(B, dr, e.data());
    const float inv = vh_inv_dr(dr);
    const int64_t n_orig = vhd_origins(T, 0, stride), n_tiles = (n_a + kVhdCpuTile - 1) / kVhdCpuTile;
#pragma omp parallel for num_threads(nth) schedule(dynamic)
    for (int64_t w = 0; w < n_orig * n_tiles; ++w) {
        const int64_t t = (w / n_tiles) * stride, p0 = (w % n_tiles) * kVhdCpuTile, p1 = std::min(n_a, p0 + kVhdCpuTile);
        int64_t* h = hist.data() + (size_t)omp_get_thread_num() * nh;
        double H[3], M[3];
        frame_box<D, PERIODIC>(hm, per_frame, t, H, M);
        for (int l = 0; l < L && t + lags[l] < T; ++l) {  // (the lags increase)
            const int64_t t2 = t + lags[l];
            for (int64_t p = p0; p < p1; ++p) {
                double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
                for (int d = 0; d < D; ++d) a[d] = (double)x[((size_t)t * A + ida[p]) * D + d];
                for (int64_t q = 0; q < n_b; ++q) {
                    if (idb[q] == ida[p]) continue;
                    for (int d = 0; d < D; ++d) b[d] = (double)x[((size_t)t2 * A + idb[q]) * D + d];
                    ++h[l * nb + vh_bin(vhd_r2<D, PERIODIC>(a, b, H, M), e.data(), B, inv)];
                }
            }
        }
    }
    std::fill(counts, counts + nh, (int64_t)0);
    for (int th = 0; th < nth; ++th)
        for (size_t i = 0; i < nh; ++i) counts[i] += hist[(size_t)th * nh + i];
    return TA_OK;
}

int vanhove_distinct(const State& s, int L, const int64_t* lags, int64_t stride, int64_t n_a, const int32_t* ida, int64_t n_b,
                     const int32_t* idb, const double* hm, bool per_frame, int B, double dr, int64_t* counts) {
    TA_PAIR_DISPATCH(vanhove_distinct_t, s, L, lags, stride, n_a, ida, n_b, idb, hm, per_frame, B, dr, counts);
}

// ---- pair and bond lifetimes (pair_math.hpp, bond_math.hpp) ---------------------------------------------------------------------------------
template <class E, int D, bool PERIODIC>
int pair_find_t(const State& s, int64_t n_a, const int32_t* ida, int64_t n_b, const int32_t* idb, bool same, int64_t stride,
                const double* hm, bool per_frame, double rc2, std::vector<int32_t>* pairs) {
    const int64_t T = s.T, A = s.A, words_b = (n_b + 63) / 64;
    const E* x = static_cast<const E*>(s.slabs[0]);
    std::vector<uint64_t> bits;
    try {
        bits.assign((size_t)n_a * (size_t)words_b, 0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
#pragma omp parallel for num_threads(s.threads > 0 ? s.threads : 1) schedule(dynamic)
    for (int64_t p = 0; p < n_a; ++p) {
        uint64_t* row = bits.data() + (size_t)p * words_b;
        for (int64_t t = 0; t < T; t += stride) {
            double H[3], M[3];
            frame_box<D, PERIODIC>(hm, per_frame, t, H, M);
            double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
            for (int d = 0; d < D; ++d) a[d] = (double)x[((size_t)t * A + ida[p]) * D + d];
            for (int64_t q = same ? p + 1 : 0; q < n_b; ++q) {
                if (idb[q] == ida[p]) continue;
                for (int d = 0; d < D; ++d) b[d] = (double)x[((size_t)t * A + idb[q]) * D + d];
                if (pair_bonded<D, PERIODIC>(a, b, H, M, rc2)) row[q >> 6] |= (uint64_t)1 << (q & 63);
            }
        }
    }
    try {
        pairs->clear();
        for (int64_t p = 0; p < n_a; ++p)
            for (int64_t w = 0; w < words_b; ++w)
                for (uint64_t m = bits[(size_t)p * words_b + w]; m; m &= m - 1) {
                    pairs->push_back(ida[p]);
                    pairs->push_back(idb[w * 64 + __builtin_ctzll(m)]);
                }
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    return TA_OK;
}

// The three sums of P packed 0/1 series: fill(n, w) sets the bits of series n in its W = ceil(T / 64) zeroed words
template <class Fill>
int lifetime_sums(const State& s, bool fft, int64_t P, double* ci, int64_t* runs, double* nb, Fill fill) {
    const int64_t T = s.T, W = (T + 63) / 64;
    const int nth = s.threads > 0 ? s.threads : 1;
    const size_t per = 3 * (size_t)T + 1;  // a thread's ci | nb | runs
    std::vector<int64_t> acc;
    std::vector<uint64_t> words;
    std::vector<double> ind;
    try {
        acc.assign((size_t)nth * per, 0);
        words.assign((size_t)nth * (size_t)(W + 1), 0);
        if (ci && fft) ind.assign((size_t)T * (size_t)P, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
#pragma omp parallel for num_threads(nth) schedule(dynamic)
    for (int64_t n = 0; n < P; ++n) {
        const int th = omp_get_thread_num();
        int64_t *a_ci = acc.data() + (size_t)th * per, *a_nb = a_ci + T, *a_runs = a_nb + T;
        uint64_t* w = words.data() + (size_t)th * (size_t)(W + 1);
        std::fill(w, w + W + 1, (uint64_t)0);  // (w[W] stays 0: the word behind the last)
        fill(n, w);
        for (int64_t j = 0; j < W; ++j)
            for (uint64_t m = w[j]; m; m &= m - 1) {
                const int64_t t = j * 64 + __builtin_ctzll(m);
                ++a_nb[t];
                if (!ind.empty()) ind[(size_t)t * P + n] = 1.0;
            }
        if (runs) {
            long long carry = 0;
            for (int64_t j = 0; j < W; ++j) {
                const uint64_t m = w[j];
                if (carry && !(m & 1)) ++a_runs[carry];
                for (uint64_t ends = m & ~(m >> 1) & ~((uint64_t)1 << 63); ends; ends &= ends - 1)
                    ++a_runs[pair_runs_word(m, __builtin_ctzll(ends), carry)];
                carry = pair_runs_carry(m, carry);
            }
            if (carry) ++a_runs[carry];
        }
        if (ci && !fft) {  // sum_t h(t) h(t + tau): the popcount of the series against itself moved down by tau
            for (int64_t tau = 0; tau < T; ++tau) {
                const int64_t jw = tau >> 6;
                const int sh = (int)(tau & 63);
                int64_t c = 0;
                for (int64_t j = 0; j + jw < W; ++j) {
                    const uint64_t moved = sh ? (w[j + jw] >> sh) | (w[j + jw + 1] << (64 - sh)) : w[j + jw];
                    c += __builtin_popcountll(w[j] & moved);
                }
                a_ci[tau] += c;
            }
        }
    }
    auto total = [&](size_t off, size_t i) {
        int64_t v = 0;
        for (int th = 0; th < nth; ++th) v += acc[(size_t)th * per + off + i];
        return v;
    };
    if (ci && !fft)
        for (int64_t k = 0; k < T; ++k) ci[k] = (double)total(0, (size_t)k);
    if (nb)
        for (int64_t t = 0; t < T; ++t) nb[t] = (double)total((size_t)T, (size_t)t);
    if (runs)
        for (int64_t l = 0; l <= T; ++l) runs[l] = total(2 * (size_t)T, (size_t)l);
    if (ci && fft) {  // the (T, P) indicator array is a slab of P atoms with dim 1
        const State v = f64_slab(s.threads, T, P, 1, ind.data());
        if (int rc = vacf_fft(v, ci, nullptr)) return rc;
        for (int64_t k = 0; k < T; ++k) ci[k] *= (double)(T - k);
    }
    return TA_OK;
}

// the box of frame t and the NAT items of a row in it, widened
template <class E, int D, bool PERIODIC, int NAT>
void bond_frame(const E* x, int64_t A, int64_t t, const int32_t* row, const double* hm, bool per_frame, double (&H)[3], double (&M)[3],
                double (&at)[NAT][3]) {
    frame_box<D, PERIODIC>(hm, per_frame, t, H, M);
    for (int i = 0; i < NAT; ++i)
        for (int d = 0; d < 3; ++d) at[i][d] = d < D ? (double)x[((size_t)t * A + row[i]) * D + d] : 0.0;
}

template <class E, int D, bool PERIODIC>
int pair_lifetime_t(const State& s, bool fft, int64_t P, const int32_t* pairs, const double* hm, bool per_frame, double rc2, double* ci,
                    int64_t* runs, double* nb) {
    const E* x = static_cast<const E*>(s.slabs[0]);
    return lifetime_sums(s, fft, P, ci, runs, nb, [&](int64_t n, uint64_t* w) {
        for (int64_t t = 0; t < s.T; ++t) {
            double H[3], M[3], at[2][3];
            bond_frame<E, D, PERIODIC, 2>(x, s.A, t, pairs + 2 * n, hm, per_frame, H, M, at);
            if (pair_bonded<D, PERIODIC>(at[0], at[1], H, M, rc2)) w[t >> 6] |= (uint64_t)1 << (t & 63);
        }
    });
}

void level_words_filter(int64_t nw, int gap, uint64_t* w, const uint64_t* S);

// the level words S (level 2) and W (level >= 1) of bond n, then hysteresis word by word and the closing of every clear bit
// of a word against the words around it (bond_math.hpp): w gets g
template <class E, int D, bool PERIODIC, int NAT>
void bond_fill(const State& s, const int32_t* row, const double* hm, bool per_frame, const BondCuts& cuts, int gap, uint64_t* w,
               uint64_t* S) {
    const int64_t T = s.T, nw = (T + 63) / 64;
    const E* x = static_cast<const E*>(s.slabs[0]);
    std::fill(S, S + nw, (uint64_t)0);
    for (int64_t t = 0; t < T; ++t) {  // (w holds the W bits first)
        double H[3], M[3], at[NAT][3];
        bond_frame<E, D, PERIODIC, NAT>(x, s.A, t, row, hm, per_frame, H, M, at);
        const int level = bond_level<D, PERIODIC, NAT>(at, H, M, cuts);
        if (level >= 1) w[t >> 6] |= (uint64_t)1 << (t & 63);
        if (level == 2) S[(size_t)(t >> 6)] |= (uint64_t)1 << (t & 63);
    }
    level_words_filter(nw, gap, w, S);
}

// w: the W bits (level >= 1) of nw words with w[nw] = 0 behind them, S: the level-2 bits: w gets g (hysteresis, then closing)
void level_words_filter(int64_t nw, int gap, uint64_t* w, const uint64_t* S) {
    bool carry = false;
    for (int64_t j = 0; j < nw; ++j) {
        w[j] = bond_hyst_word(S[(size_t)j], w[j], carry);
        carry = w[j] >> 63;
    }
    if (!gap) return;
    uint64_t prev = 0;  // (the word before, as it was before its own closing)
    for (int64_t j = 0; j < nw; ++j) {
        const uint64_t cur = w[j], next = w[j + 1];  // (w[nw] is 0)
        uint64_t add = 0;
        for (uint64_t m = ~cur; m; m &= m - 1) {
            const int i = __builtin_ctzll(m);
            if (bond_close_bit(prev, cur, next, i, gap)) add |= (uint64_t)1 << i;
        }
        w[j] = cur | add, prev = cur;  // (no bit at or behind frame T is filled: nothing is set above it)
    }
}

template <class E, int D, bool PERIODIC>
int bond_lifetime_t(const State& s, bool fft, int64_t P, int n_at, const int32_t* atoms, const double* hm, bool per_frame,
                    const BondCuts& cuts, int gap, double* ci, int64_t* runs, double* nb) {
    const size_t nw = (size_t)((s.T + 63) / 64);
    std::vector<uint64_t> S;  // a thread's level-2 words
    try {
        S.assign((size_t)(s.threads > 0 ? s.threads : 1) * nw, 0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    return lifetime_sums(s, fft, P, ci, runs, nb, [&](int64_t n, uint64_t* w) {
        uint64_t* Sw = S.data() + (size_t)omp_get_thread_num() * nw;
        if (n_at == 3) bond_fill<E, D, PERIODIC, 3>(s, atoms + 3 * n, hm, per_frame, cuts, gap, w, Sw);
        else bond_fill<E, D, PERIODIC, 2>(s, atoms + 2 * n, hm, per_frame, cuts, gap, w, Sw);
    });
}

// The series of the observed item idq against ALL reference items ida (one with its own id does not count): the level words
// by shell_level (Sw: nw words for the level-2 bits), then bond_fill's filter: w gets g
template <class E, int D, bool PERIODIC>
void shell_fill(const E* x, int64_t T, int64_t A, int64_t n_a, const int32_t* ida, int32_t idq, const double* hm, bool per_frame,
                const BondCuts& cuts, int gap, uint64_t* Sw, uint64_t* w) {
    const int64_t nw = (T + 63) / 64;
    std::fill(Sw, Sw + nw, (uint64_t)0);
    for (int64_t t = 0; t < T; ++t) {
        double H[3], M[3], a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
        frame_box<D, PERIODIC>(hm, per_frame, t, H, M);
        for (int d = 0; d < D; ++d) b[d] = (double)x[((size_t)t * A + idq) * D + d];
        bool form = false, brk = false;
        for (int64_t p = 0; p < n_a; ++p) {
            if (ida[p] == idq) continue;
            for (int d = 0; d < D; ++d) a[d] = (double)x[((size_t)t * A + ida[p]) * D + d];
            const double r2 = vhd_r2<D, PERIODIC>(a, b, H, M);
            form |= r2 < cuts.rc2, brk |= r2 < cuts.rb2;
        }
        const int level = shell_level(form, brk);
        if (level >= 1) w[t >> 6] |= (uint64_t)1 << (t & 63);
        if (level == 2) Sw[t >> 6] |= (uint64_t)1 << (t & 63);
    }
    level_words_filter(nw, gap, w, Sw);
}

// shell_fill per observed item; OpenMP over the observed items (lifetime_sums)
template <class E, int D, bool PERIODIC>
int shell_residence_t(const State& s, bool fft, int64_t n_a, const int32_t* ida, int64_t n_b, const int32_t* idb, const double* hm,
                      bool per_frame, const BondCuts& cuts, int gap, double* ci, int64_t* runs, double* nb) {
    const int64_t T = s.T, A = s.A, nw = (T + 63) / 64;
    const E* x = static_cast<const E*>(s.slabs[0]);
    std::vector<uint64_t> S;  // a thread's level-2 words
    try {
        S.assign((size_t)(s.threads > 0 ? s.threads : 1) * (size_t)nw, 0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    return lifetime_sums(s, fft, n_b, ci, runs, nb, [&](int64_t n, uint64_t* w) {
        shell_fill<E, D, PERIODIC>(x, T, A, n_a, ida, idb[n], hm, per_frame, cuts, gap, S.data() + (size_t)omp_get_thread_num() * (size_t)nw, w);
    });
}

// The gated lag sums behind shell_residence_t's series g of every observed item (runs, nb by lifetime_sums), for ta_shell_msd
// and ta_shell_orient: behind each item's fill its NS sums over the lags 0 ... L with shell_msd_math.hpp's gates, as
// shell_gate_walk: a plain loop over the origins inside, left(s) from one walk down the frames.  item(n, thread) prepares item
// n and returns its term(acc, t, t + k), which adds one term onto the NS sums acc.  A thread adds into sums and counts of its
// own; the threads' sums are added in thread order (exact inputs: any order gives the same bits).
template <class E, int D, bool PERIODIC, int NS, class Item>
int shell_gated_sums(const State& s, int condition, int64_t L, int64_t n_a, const int32_t* ida, int64_t n_b, const int32_t* idb, const double* hm,
                     bool per_frame, const BondCuts& cuts, int gap, double* sums, int64_t* count, int64_t* runs, double* nb, Item item) {
    const int64_t T = s.T, A = s.A, nw = (T + 63) / 64;
    const int nth = s.threads > 0 ? s.threads : 1;
    const E* x = static_cast<const E*>(s.slabs[0]);
    const size_t n1 = (size_t)(L + 1) * NS, n2 = (size_t)L + 1;
    std::vector<uint64_t> S;
    std::vector<double> acc;
    std::vector<int64_t> cnt, left;
    try {
        S.assign((size_t)nth * (size_t)nw, 0);
        acc.assign((size_t)nth * n1, 0.0);
        cnt.assign((size_t)nth * n2, 0);
        left.assign((size_t)nth * (size_t)(T + 1), 0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    const int rc = lifetime_sums(s, false, n_b, nullptr, runs, nb, [&](int64_t n, uint64_t* w) {
        const int th = omp_get_thread_num();
        shell_fill<E, D, PERIODIC>(x, T, A, n_a, ida, idb[n], hm, per_frame, cuts, gap, S.data() + (size_t)th * (size_t)nw, w);
        if (!sums && !count) return;
        double* a_s = acc.data() + (size_t)th * n1;
        int64_t *a_n = cnt.data() + (size_t)th * n2, *lf = left.data() + (size_t)th * (size_t)(T + 1);
        auto inside = [&](int64_t t) { return (w[t >> 6] >> (t & 63)) & 1; };
        lf[T] = 0;
        for (int64_t t = T - 1; t >= 0; --t) lf[t] = inside(t) ? lf[t + 1] + 1 : 0;
        auto term = item(n, th);
        for (int64_t t = 0; t < T; ++t) {
            if (!inside(t)) continue;
            const int64_t k_end = condition == SHELL_CONTINUOUS ? std::min(lf[t], L + 1) : std::min(T - t, L + 1);
            for (int64_t k = 0; k < k_end; ++k) {
                if (condition == SHELL_ENDPOINTS && !inside(t + k)) continue;
                ++a_n[k];
                term(a_s + k * NS, t, t + k);
            }
        }
    });
    if (rc) return rc;
    for (size_t i = 0; sums && i < n1; ++i) {
        double v = 0.0;
        for (int th = 0; th < nth; ++th) v += acc[(size_t)th * n1 + i];
        sums[i] = v;
    }
    for (size_t i = 0; count && i < n2; ++i) {
        int64_t v = 0;
        for (int th = 0; th < nth; ++th) v += cnt[(size_t)th * n2 + i];
        count[i] = v;
    }
    return TA_OK;
}

// ta_shell_msd: the term is shell_msd_add per axis, fma(d, d, acc), as k_shell_msd's
template <class E, int D, bool PERIODIC>
int shell_msd_t(const State& s, int condition, int64_t L, int64_t n_a, const int32_t* ida, int64_t n_b, const int32_t* idb, const double* hm,
                bool per_frame, const BondCuts& cuts, int gap, double* sums, int64_t* count, int64_t* runs, double* nb) {
    const int64_t A = s.A;
    const E* x = static_cast<const E*>(s.slabs[0]);
    return shell_gated_sums<E, D, PERIODIC, D>(s, condition, L, n_a, ida, n_b, idb, hm, per_frame, cuts, gap, sums, count, runs, nb,
                                               [&](int64_t n, int) {
                                                   const E* xq = x + (size_t)idb[n] * D;
                                                   return [=](double* acc, int64_t t, int64_t t2) {
                                                       for (int d = 0; d < D; ++d)
                                                           acc[d] = shell_msd_add(acc[d], (double)xq[(size_t)t * A * D + d], (double)xq[(size_t)t2 * A * D + d]);
                                                   };
                                               });
}

// ta_shell_orient: u of the item's vector in every frame by orient_math.hpp's sequence with the distance pass's box, kept per
// thread; the term is shell_orient_math.hpp's, as k_shell_orient's
template <class E, bool PERIODIC, int MODE>
int shell_orient_t(const State& s, int condition, int64_t L, const int32_t* index, int64_t n_a, const int32_t* ida, int64_t n_b,
                   const int32_t* idb, const double* hm, bool per_frame, const BondCuts& cuts, int gap, double* sums, int64_t* count,
                   int64_t* runs, double* nb) {
    const int64_t T = s.T, A = s.A;
    constexpr int K = MODE == ORIENT_BOND ? 2 : 3;
    const E* x = static_cast<const E*>(s.slabs[0]);
    std::vector<double> U;
    try {
        if (sums || count) U.assign((size_t)(s.threads > 0 ? s.threads : 1) * (size_t)T * 3, 0.0);
    } catch (const std::bad_alloc&) {
        return TA_E_NOMEM;
    }
    return shell_gated_sums<E, 3, PERIODIC, 2>(s, condition, L, n_a, ida, n_b, idb, hm, per_frame, cuts, gap, sums, count, runs, nb,
                                               [&](int64_t n, int th) {
        double* u = U.data() + (size_t)th * (size_t)T * 3;
        const int32_t* row = index + n * K;
        for (int64_t t = 0; t < T; ++t) {
            double at[3][3] = {};
            for (int j = 0; j < K; ++j)
                for (int d = 0; d < 3; ++d) at[j][d] = (double)x[((size_t)t * A + (size_t)row[j]) * 3 + d];
            OrientBox bx{};
            if (PERIODIC) bx = shell_orient_box(hm + (per_frame ? t * 6 : 0));
            shell_orient_unit<MODE, PERIODIC>(at[0], at[1], at[2], bx, *reinterpret_cast<double(*)[3]>(u + 3 * t));
        }
        return [=](double* acc, int64_t t, int64_t t2) {
            const double *a = u + 3 * t, *b = u + 3 * t2;
            shell_orient_add(acc[0], acc[1], shell_orient_dot(a[0], a[1], a[2], b[0], b[1], b[2]));
        };
    });
}

int pair_find(const State& s, int64_t n_a, const int32_t* ida, int64_t n_b, const int32_t* idb, bool same, int64_t stride,
              const double* hm, bool per_frame, double rc2, std::vector<int32_t>* pairs) {
    TA_PAIR_DISPATCH(pair_find_t, s, n_a, ida, n_b, idb, same, stride, hm, per_frame, rc2, pairs);
}
int pair_lifetime(const State& s, bool fft, int64_t P, const int32_t* pairs, const double* hm, bool per_frame, double rc2, double* ci,
                  int64_t* runs, double* nb) {
    TA_PAIR_DISPATCH(pair_lifetime_t, s, fft, P, pairs, hm, per_frame, rc2, ci, runs, nb);
}
int bond_lifetime(const State& s, bool fft, int64_t P, int n_at, const int32_t* atoms, const double* hm, bool per_frame,
                  const BondCuts& cuts, int gap, double* ci, int64_t* runs, double* nb) {
    TA_PAIR_DISPATCH(bond_lifetime_t, s, fft, P, n_at, atoms, hm, per_frame, cuts, gap, ci, runs, nb);
}
// (the templates take the shared arguments of a shell call one by one)
#define TA_SHELL_ITEMS c.n_a, c.ida, c.n_b, c.idb, c.hm, c.per_frame, *c.cuts, c.gap
int shell_residence(const State& s, bool fft, const ShellItems& c, double* ci, int64_t* runs, double* nb) {
    const double* hm = c.hm;
    TA_PAIR_DISPATCH(shell_residence_t, s, fft, TA_SHELL_ITEMS, ci, runs, nb);
}
int shell_msd(const State& s, int condition, int64_t max_lag, const ShellItems& c, double* sums, int64_t* count, int64_t* runs, double* nb) {
    const double* hm = c.hm;
    TA_PAIR_DISPATCH(shell_msd_t, s, condition, max_lag, TA_SHELL_ITEMS, sums, count, runs, nb);
}
#undef TA_PAIR_DISPATCH
int shell_orient(const State& s, int condition, int64_t max_lag, int mode, const int32_t* index, const ShellItems& c, double* sums,
                 int64_t* count, int64_t* runs, double* nb) {
    const double* hm = c.hm;
#define TA_SO_ARGS s, condition, max_lag, index, TA_SHELL_ITEMS, sums, count, runs, nb
#define TA_SO_MODE(E, P)                                                                 \
    return mode == ORIENT_BOND       ? shell_orient_t<E, P, ORIENT_BOND>(TA_SO_ARGS)     \
           : mode == ORIENT_BISECTOR ? shell_orient_t<E, P, ORIENT_BISECTOR>(TA_SO_ARGS) \
                                     : shell_orient_t<E, P, ORIENT_NORMAL>(TA_SO_ARGS)
    if (s.dtype == TA_F32) {
        if (hm) TA_SO_MODE(float, true);
        TA_SO_MODE(float, false);
    }
    if (hm) TA_SO_MODE(double, true);
    TA_SO_MODE(double, false);
#undef TA_SO_MODE
#undef TA_SO_ARGS
#undef TA_SHELL_ITEMS
}

template <class E>
int compound_t(const State& s, int64_t C, const int64_t* off, const int32_t* members, const double* w, const double* u,
               double* out) {
    const int64_t T = s.T, A = s.A;
    const int D = s.D;
    const E* x = static_cast<const E*>(s.slabs[0]);
    std::vector<double> F;
    if (u) {
        try {
            F.assign((size_t)T * D, 0.0);
        } catch (const std::bad_alloc&) {
            return TA_E_NOMEM;
        }
#pragma omp parallel for num_threads(s.threads) schedule(static)
        for (int64_t t = 0; t < T; ++t)
            for (int64_t a = 0; a < A; ++a)
                for (int d = 0; d < D; ++d) F[(size_t)t * D + d] = std::fma(u[a], (double)x[((size_t)t * A + a) * D + d], F[(size_t)t * D + d]);
    }
#pragma omp parallel for num_threads(s.threads) schedule(dynamic, 16)
    for (int64_t c = 0; c < C; ++c) {
        double g = 0.0;
        for (int64_t i = off[c]; i < off[c + 1]; ++i) g += w ? w[i] : 1.0;
        for (int64_t t = 0; t < T; ++t) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int64_t i = off[c]; i < off[c + 1]; ++i) {
                const double wi = w ? w[i] : 1.0;
                const E* row = x + ((size_t)t * A + members[i]) * D;
                for (int d = 0; d < D; ++d) acc[d] = i == off[c] ? wi * (double)row[d] : std::fma(wi, (double)row[d], acc[d]);
            }
            double* o = out + ((size_t)t * C + c) * D;
            for (int d = 0; d < D; ++d) o[d] = u ? std::fma(-g, F[(size_t)t * D + d], acc[d]) : acc[d];
        }
    }
    return TA_OK;
}

int compound(const State& s, int64_t C, const int64_t* off, const int32_t* members, const double* w, const double* u, double* out) {
    return s.dtype == TA_F32 ? compound_t<float>(s, C, off, members, w, u, out) : compound_t<double>(s, C, off, members, w, u, out);
}

template <class E>
void unwrap_t(const State& s, int slab, const BoxTable& box, const int* axes) {
    const int64_t T = s.T, A = s.A, tp = box.per_frame ? box.tpitch : 0;
    const int D = s.D;
    E* p = static_cast<E*>(s.slabs[slab]);
    const double* tab = box.tab.data();
    auto at = [&](int row, int64_t t) { return tab[row * box.tpitch + (tp ? t : 0)]; };
#pragma omp parallel for num_threads(s.threads) schedule(static)
    for (int64_t a = 0; a < A; ++a) {
        double prev[3] = {0.0, 0.0, 0.0};
        int n[3] = {0, 0, 0};
        for (int64_t t = 0; t < T; ++t) {
            E* row = p + ((size_t)t * A + a) * D;
            double x[3] = {0.0, 0.0, 0.0}, f[3];
            for (int d = 0; d < D; ++d) x[d] = (double)row[d];
            if (box.triclinic) {
                f[0] = x[0] * at(6, t) + x[1] * at(7, t) + x[2] * at(9, t);
                f[1] = x[1] * at(8, t) + x[2] * at(10, t);
                f[2] = x[2] * at(11, t);
            } else {
                for (int d = 0; d < D; ++d) f[d] = x[d] * at(6 + diag_row(axes[d]), t);
            }
            if (t)
                for (int d = 0; d < D; ++d) n[d] += (int)std::nearbyint(f[d] - prev[d]);  // (round-half-even)
            for (int d = 0; d < D; ++d) prev[d] = f[d];
            if (box.triclinic) {
                const double n0 = n[0], n1 = n[1], n2 = n[2];
                row[0] = (E)(x[0] - (n0 * at(0, t) + n1 * at(1, t) + n2 * at(3, t)));
                row[1] = (E)(x[1] - (n1 * at(2, t) + n2 * at(4, t)));
                row[2] = (E)(x[2] - n2 * at(5, t));
            } else {
                for (int d = 0; d < D; ++d) row[d] = (E)(x[d] - (double)n[d] * at(diag_row(axes[d]), t));
            }
        }
    }
}

void unwrap(const State& s, int slab, const BoxTable& box, const int* axes) {
    if (s.dtype == TA_F32) unwrap_t<float>(s, slab, box, axes);
    else unwrap_t<double>(s, slab, box, axes);
}

}  // namespace cpu
}  // namespace ta
