// unwrap_box.hpp — the per-frame box table of ta_unwrap, shared by the GPU path (api.hip, group.hip) and the CPU backend.
//
// ts.dimensions = [a, b, c, alpha, beta, gamma] -> H, the 3x3 matrix whose rows are the box vectors, by MDAnalysis'
// triclinic_vectors formula in float64 (lower-triangular; diagonal when all three angles are exactly 90), and its
// inverse M = H^-1 (lower-triangular as well).  The table keeps their six non-zero entries each, as 12 rows of tpitch
// doubles:
//   row 0..5   H00 H10 H11 H20 H21 H22
//   row 6..11  M00 M10 M11 M20 M21 M22
// element t of a row = frame t (per_frame), or the one constant box at t = 0 (tpitch 1).  The diagonal entry of axis a is
// row diag_row(a) (H) and 6 + diag_row(a) (M).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ta {

constexpr int kBoxRows = 12;
inline constexpr int diag_row(int axis) { return axis * (axis + 3) / 2; }  // 0, 2, 5

struct BoxTable {
    std::vector<double> tab;  // kBoxRows * tpitch
    int64_t tpitch = 1;
    bool per_frame = false;   // some frame differs from frame 0
    bool triclinic = false;   // some frame is not orthogonal
};

// H (six entries, row order above) of one frame; "" or why the box is rejected
inline std::string box_vectors(const double* d, double* h) {
    for (int i = 0; i < 3; ++i)
        if (!(d[i] > 0.0) || !std::isfinite(d[i])) return "box length <= 0 or not finite";
    const double al = d[3], be = d[4], ga = d[5];
    if (!(al > 0.0 && al < 180.0 && be > 0.0 && be < 180.0 && ga > 0.0 && ga < 180.0))
        return "box angle outside (0, 180) degrees";
    std::memset(h, 0, 6 * sizeof(double));
    if (al == 90.0 && be == 90.0 && ga == 90.0) {
        h[0] = d[0], h[2] = d[1], h[5] = d[2];
        return "";
    }
    const double deg = 3.141592653589793 / 180.0;  // np.deg2rad
    const double ca = al == 90.0 ? 0.0 : std::cos(al * deg);
    const double cb = be == 90.0 ? 0.0 : std::cos(be * deg);
    const double cg = ga == 90.0 ? 0.0 : std::cos(ga * deg);
    const double sg = ga == 90.0 ? 1.0 : std::sin(ga * deg);
    h[0] = d[0];
    h[1] = d[1] * cg;
    h[2] = d[1] * sg;
    h[3] = d[2] * cb;
    h[4] = d[2] * (ca - cb * cg) / sg;
    h[5] = std::sqrt(d[2] * d[2] - h[3] * h[3] - h[4] * h[4]);
    if (!(h[5] > 0.0)) return "box angles do not make a box";
    return "";
}

// The table of n_frames rows of dims ((n_frames, 6)); per-frame tables get tpitch = n_frames rounded up to `round`.
// axes: dim entries in 0..2.  Returns "" or the reason for TA_E_INVALID.
inline std::string box_table(const double* dims, int64_t n_frames, int dim, const int* axes, int64_t round, BoxTable* out) {
    for (int d = 0; d < dim; ++d)
        if (axes[d] < 0 || axes[d] > 2) return "axes: every entry must be 0, 1 or 2";
    out->per_frame = false, out->triclinic = false;
    for (int64_t t = 0; t < n_frames; ++t) {
        const double* d = dims + 6 * t;
        if (t && std::memcmp(d, dims, 6 * sizeof(double))) out->per_frame = true;
        if (!(d[3] == 90.0 && d[4] == 90.0 && d[5] == 90.0)) out->triclinic = true;
    }
    if (out->triclinic && !(dim == 3 && axes[0] == 0 && axes[1] == 1 && axes[2] == 2))
        return "a non-orthogonal box needs the three columns x, y, z (axes {0, 1, 2})";
    const int64_t n = out->per_frame ? n_frames : 1;
    out->tpitch = out->per_frame ? (n_frames + round - 1) / round * round : 1;
    out->tab.assign((size_t)kBoxRows * out->tpitch, 0.0);
    for (int64_t t = 0; t < n; ++t) {
        double h[6];
        const std::string why = box_vectors(dims + 6 * t, h);
        if (!why.empty()) return why + " in frame " + std::to_string(t);
        double m[6];
        m[0] = 1.0 / h[0];
        m[2] = 1.0 / h[2];
        m[5] = 1.0 / h[5];
        m[1] = -h[1] * m[0] / h[2];
        m[4] = -h[4] * m[2] / h[5];
        m[3] = -(h[3] * m[0] + h[4] * m[1]) / h[5];
        for (int k = 0; k < 6; ++k) {
            out->tab[(size_t)k * out->tpitch + t] = h[k];
            out->tab[(size_t)(6 + k) * out->tpitch + t] = m[k];
        }
    }
    return "";  // (a constant box: every frame is frame 0, checked above)
}

}  // namespace ta
