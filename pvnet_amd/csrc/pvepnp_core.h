// pvepnp_core.h -- EPnP for one image, written as a sequence of lane phases.
//
// OpenCV modules/calib3d/src/epnp.cpp (Lepetit, Moreno-Noguer, Fua, IJCV 2009) restated in
// fp64; include/pvpose.h lists the steps and this project's conventions on top of them.
//
// Form: epnp_image() is a list of PVE_PHASE(lane) { ... } blocks.  On the device a phase is
// the body run by the block's 64 lanes followed by a barrier; everything that lives across a
// phase boundary is in the Epnp structure (LDS), and the code between phases reads only that,
// so control flow is uniform.  Compiled for the host (no HIP headers needed) a phase is a loop
// over the 64 lanes, which runs the very same arithmetic on a CPU for checking.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PVE_FN __device__ inline
#define PVE_PHASE(lane) for (int lane = threadIdx.x, once_ = 1; once_; once_ = 0, __syncthreads())
#else
#define PVE_FN inline
#define PVE_PHASE(lane) for (int lane = 0; lane < 64; ++lane)
#endif

namespace pve {

constexpr int kLanes = 64;
constexpr int kMinPts = 6, kMaxPts = 64;
constexpr int kStatusOk = 0, kStatusDegenerate = 1;   // PV_EPNP_OK, PV_EPNP_DEGENERATE
constexpr int kJacobiSweeps = 30;
constexpr double kPlanarRatio = 1e-12;   // smallest / largest PCA eigenvalue of the model
constexpr double kRankRatio = 1e-10;     // smallest / largest singular value of the Arun matrix
constexpr double kTiny = 1e-30;          // off-diagonal entries below kTiny * trace are zero

struct Epnp {
    double pw[kMaxPts][3];      // model points
    double al[kMaxPts][4];      // barycentric coordinates
    double du[kMaxPts], dv[kMaxPts];   // uc - u, vc - v
    union {   // the Jacobi iteration is over (its result copied to v) before the candidates start
        struct {
            double A[2][144], V[2][144];   // the 12x12 Jacobi iteration, double buffered
        };
        double pc[3][kMaxPts][3];   // camera-frame points of the three candidates, then their errors
    };
    double cam[4];              // fu, fv, uc, vc
    double c0[3], cov[9];
    double cws[4][3], ccinv[3][3];
    double jc[12], js[12];      // the step's rotation of every index: new_i = jc_i * i + js_i * partner_i
    int jp[12], rot[6], nrot;
    int vsel[4];
    double v[4][12];
    double L[6][10], rho[6];
    double ls[3][6][6];         // per candidate: the least-squares system [A | b]
    double ccs[3][4][3];
    double pc0[3][3], abt[3][9];
    double R[3][9], t[3][3], err[3];
    int bad[3];
    int degenerate;
};

struct Out {
    double Rt[12], rt6[6], cand_err[3];
    int status, n_used;
};

// cyclic Jacobi on a symmetric 3x3 (serial): eigenvalues w, eigenvectors in the columns of U
PVE_FN void jacobi_eig3(const double a_in[9], double w[3], double U[9]) {
    double a[9];
    for (int i = 0; i < 9; ++i) { a[i] = a_in[i]; U[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    const double tiny = kTiny * (fabs(a[0]) + fabs(a[4]) + fabs(a[8]));
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        int nrot = 0;
        for (int p = 0; p < 2; ++p) {
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p * 3 + q];
                if (!(fabs(apq) > tiny)) continue;
                ++nrot;
                const double th = (a[q * 3 + q] - a[p * 3 + p]) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {   // columns: A J
                    const double x = a[k * 3 + p], y = a[k * 3 + q];
                    a[k * 3 + p] = c * x - s * y;
                    a[k * 3 + q] = s * x + c * y;
                }
                for (int k = 0; k < 3; ++k) {   // rows: J^T (A J)
                    const double x = a[p * 3 + k], y = a[q * 3 + k];
                    a[p * 3 + k] = c * x - s * y;
                    a[q * 3 + k] = s * x + c * y;
                }
                a[p * 3 + q] = a[q * 3 + p] = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double x = U[k * 3 + p], y = U[k * 3 + q];
                    U[k * 3 + p] = c * x - s * y;
                    U[k * 3 + q] = s * x + c * y;
                }
            }
        }
        if (nrot == 0) break;
    }
    w[0] = a[0]; w[1] = a[4]; w[2] = a[8];
}

// one-sided (Hestenes) Jacobi SVD of a 3x3, B = U diag(s) V^T -> R = U V^T; false if B's smallest
// singular value is <= kRankRatio of its largest (the points are coplanar: no rotation is defined)
PVE_FN bool polar_rotation3(const double B[9], double R[9]) {
    double g[9], v[9];
    for (int i = 0; i < 9; ++i) { g[i] = B[i]; v[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        int nrot = 0;
        for (int p = 0; p < 2; ++p) {
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int k = 0; k < 3; ++k) {
                    al += g[k * 3 + p] * g[k * 3 + p];
                    be += g[k * 3 + q] * g[k * 3 + q];
                    ga += g[k * 3 + p] * g[k * 3 + q];
                }
                if (!(fabs(ga) > 4.0 * DBL_EPSILON * sqrt(al * be))) continue;
                ++nrot;
                const double ze = (be - al) / (2.0 * ga);
                const double t = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(ze * ze + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double x = g[k * 3 + p], y = g[k * 3 + q];
                    g[k * 3 + p] = c * x - s * y;
                    g[k * 3 + q] = s * x + c * y;
                    const double xv = v[k * 3 + p], yv = v[k * 3 + q];
                    v[k * 3 + p] = c * xv - s * yv;
                    v[k * 3 + q] = s * xv + c * yv;
                }
            }
        }
        if (nrot == 0) break;
    }
    double sg[3], smax = 0.0;
    int km = 0;   // the smallest singular value's column
    for (int k = 0; k < 3; ++k) {
        sg[k] = sqrt(g[k] * g[k] + g[3 + k] * g[3 + k] + g[6 + k] * g[6 + k]);
        smax = fmax(smax, sg[k]);
        if (sg[k] < sg[km]) km = k;
    }
    if (!(sg[km] > kRankRatio * smax)) return false;
    // U: the two larger columns normalised; the smallest is their cross product, signed as the
    // column itself (orthonormal however small that singular value is, as LAPACK's U)
    const int ka = (km + 1) % 3, kb = (km + 2) % 3;
    double u[9];
    for (int i = 0; i < 3; ++i) {
        u[i * 3 + ka] = g[i * 3 + ka] / sg[ka];
        u[i * 3 + kb] = g[i * 3 + kb] / sg[kb];
    }
    const double cx = u[3 + ka] * u[6 + kb] - u[6 + ka] * u[3 + kb];
    const double cy = u[6 + ka] * u[kb] - u[ka] * u[6 + kb];
    const double cz = u[ka] * u[3 + kb] - u[3 + ka] * u[kb];
    const double sgn = g[km] * cx + g[3 + km] * cy + g[6 + km] * cz < 0.0 ? -1.0 : 1.0;
    u[km] = sgn * cx;
    u[3 + km] = sgn * cy;
    u[6 + km] = sgn * cz;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double r = 0.0;
            for (int k = 0; k < 3; ++k) r += u[i * 3 + k] * v[j * 3 + k];
            R[i * 3 + j] = r;
        }
    return true;
}

// least squares min |A x - b| by Householder QR; the system is a[6][6] with b in column n
PVE_FN void ls_solve6(double a[6][6], int n, double x[5]) {
    for (int k = 0; k < n; ++k) {
        double nrm = 0.0;
        for (int i = k; i < 6; ++i) nrm += a[i][k] * a[i][k];
        nrm = sqrt(nrm);
        const double alpha = a[k][k] > 0.0 ? -nrm : nrm;
        const double vk = a[k][k] - alpha;
        double vtv = vk * vk;
        for (int i = k + 1; i < 6; ++i) vtv += a[i][k] * a[i][k];
        if (vtv > 0.0) {
            for (int col = k + 1; col <= n; ++col) {   // the remaining columns and b
                double d = vk * a[k][col];
                for (int i = k + 1; i < 6; ++i) d += a[i][k] * a[i][col];
                const double f = 2.0 * d / vtv;
                a[k][col] -= f * vk;
                for (int i = k + 1; i < 6; ++i) a[i][col] -= f * a[i][k];
            }
        }
        a[k][k] = alpha;
    }
    for (int k = n - 1; k >= 0; --k) {
        double s = a[k][n];
        for (int j = k + 1; j < n; ++j) s -= a[k][j] * x[j];
        x[k] = s / a[k][k];
    }
}

// cv2.Rodrigues(R) -> rvec, as oracle/pnp.py::rodrigues_mat_to_vec restates it
PVE_FN void rodrigues_to_vec(const double R[9], double r[3]) {
    const double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    const double c = fmin(fmax((R[0] + R[4] + R[8] - 1.0) * 0.5, -1.0), 1.0);
    const double th = acos(c);
    if (s < 1e-5) {
        if (c > 0) { r[0] = r[1] = r[2] = 0.0; return; }
        int m = 0;
        if (R[4] > R[m * 4]) m = 1;
        if (R[8] > R[m * 4]) m = 2;
        double k[3];
        k[m] = sqrt(fmax((R[m * 4] + 1.0) * 0.5, 0.0));
        for (int i = 0; i < 3; ++i)
            if (i != m) k[i] = (R[m * 3 + i] + R[i * 3 + m]) * 0.25 / k[m];
        const double n = sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
        for (int i = 0; i < 3; ++i) r[i] = k[i] / n * th;
        return;
    }
    const double vth = 1.0 / (2.0 * s) * th;
    r[0] = rx * vth;
    r[1] = ry * vth;
    r[2] = rz * vth;
}

// cv2.Rodrigues(rvec) -> R
PVE_FN void rodrigues_to_mat(const double r[3], double R[9]) {
    const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (th < DBL_EPSILON) {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double k[3] = {r[0] / th, r[1] / th, r[2] / th};
    const double c = cos(th), s = sin(th);
    const double kx[9] = {0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = (i == j ? c : 0.0) + (1.0 - c) * k[i] * k[j] + s * kx[i * 3 + j];
}

// entry c (0..11) of the two rows point i contributes to M: column 3 j + a of control point j
PVE_FN void m_rows(const Epnp &S, int i, int c, double *r1, double *r2) {
    const int j = c / 3, a = c - 3 * j;
    const double al = S.al[i][j];
    *r1 = a == 0 ? al * S.cam[0] : a == 2 ? al * S.du[i] : 0.0;
    *r2 = a == 1 ? al * S.cam[1] : a == 2 ? al * S.dv[i] : 0.0;
}

// the pairs of step r of a round-robin over 12 indices: 6 disjoint pairs, 11 steps reach all 66
PVE_FN void jacobi_pair(int r, int k, int *p, int *q) {
    int a, b;
    if (k == 0) { a = 11; b = r; }
    else { a = (r + k) % 11; b = (r + 11 - k) % 11; }
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// cv2's find_betas_approx_N (N = n + 1) and gauss_newton: five iterations
PVE_FN void solve_betas(Epnp &S, int n, double be[4]) {
    double (*a)[6] = S.ls[n];
    double x[5];
    const int c1[4] = {0, 1, 3, 6};
    const int nc = n == 0 ? 4 : n == 1 ? 3 : 5;
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < nc; ++j) a[i][j] = S.L[i][n == 0 ? c1[j] : j];
        a[i][nc] = S.rho[i];
    }
    ls_solve6(a, nc, x);
    be[0] = sqrt(fabs(x[0]));
    be[1] = be[2] = be[3] = 0.0;
    if (n == 0) {
        const double sg = x[0] < 0.0 ? -1.0 : 1.0;
        for (int k = 1; k < 4; ++k) be[k] = sg * x[k] / be[0];
    } else {
        if (x[0] < 0.0) be[1] = x[2] < 0.0 ? sqrt(-x[2]) : 0.0;
        else be[1] = x[2] > 0.0 ? sqrt(x[2]) : 0.0;
        if (x[1] < 0.0) be[0] = -be[0];
        if (n == 2) be[2] = x[3] / be[0];
    }
    for (int it = 0; it < 5; ++it) {
        const double b0 = be[0], b1 = be[1], b2 = be[2], b3 = be[3];
        for (int i = 0; i < 6; ++i) {
            const double *l = S.L[i];
            a[i][0] = 2.0 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3;
            a[i][1] = l[1] * b0 + 2.0 * l[2] * b1 + l[4] * b2 + l[7] * b3;
            a[i][2] = l[3] * b0 + l[4] * b1 + 2.0 * l[5] * b2 + l[8] * b3;
            a[i][3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2.0 * l[9] * b3;
            a[i][4] = S.rho[i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 + l[4] * b1 * b2 +
                                  l[5] * b2 * b2 + l[6] * b0 * b3 + l[7] * b1 * b3 + l[8] * b2 * b3 + l[9] * b3 * b3);
        }
        ls_solve6(a, 4, x);
        for (int k = 0; k < 4; ++k) be[k] += x[k];
    }
}

PVE_FN void degenerate_out(Out &o) {
    for (int i = 0; i < 12; ++i) o.Rt[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 6; ++i) o.rt6[i] = 0.0;
    o.status = kStatusDegenerate;
}

// One image.  p3 [pn][3], K [3][3], image points from p2d64 (if given) or p2d, both [pn][2].
// The result lands in `out` in lane 0's last phase (on the device: valid in lane 0 only).
PVE_FN void epnp_image(Epnp &S, int pn, const double *p3, const double *K, const float *p2d, const double *p2d64,
                       Out &out) {
    PVE_PHASE(lane) {
        if (lane < pn) {
            for (int k = 0; k < 3; ++k) S.pw[lane][k] = p3[lane * 3 + k];
            const double u = p2d64 ? p2d64[lane * 2] : (double)p2d[lane * 2];
            const double v = p2d64 ? p2d64[lane * 2 + 1] : (double)p2d[lane * 2 + 1];
            S.du[lane] = K[2] - u;
            S.dv[lane] = K[5] - v;
        }
        if (lane == 0) {
            S.cam[0] = K[0]; S.cam[1] = K[4]; S.cam[2] = K[2]; S.cam[3] = K[5];
            S.degenerate = 0;
        }
    }
    // ---- 1. control points: the centroid and the model's PCA axes
    PVE_PHASE(lane) {
        if (lane < 3) {
            double s = 0.0;
            for (int i = 0; i < pn; ++i) s += S.pw[i][lane];
            S.c0[lane] = s / pn;
        }
    }
    PVE_PHASE(lane) {
        if (lane < 9) {
            const int a = lane / 3, b = lane - 3 * a, lo = a < b ? a : b, hi = a < b ? b : a;
            double s = 0.0;
            for (int i = 0; i < pn; ++i) s += (S.pw[i][lo] - S.c0[lo]) * (S.pw[i][hi] - S.c0[hi]);
            S.cov[lane] = s;
        }
    }
    PVE_PHASE(lane) {
        if (lane == 0) {
            double w[3], U[9];
            jacobi_eig3(S.cov, w, U);
            int o[3] = {0, 1, 2};   // descending eigenvalue, ties to the lower index
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2 - i; ++j)
                    if (w[o[j + 1]] > w[o[j]]) { const int t = o[j]; o[j] = o[j + 1]; o[j + 1] = t; }
            if (!(w[o[2]] > kPlanarRatio * w[o[0]])) S.degenerate = 1;
            double C[9];   // columns c_j - c_0
            for (int k = 0; k < 3; ++k) S.cws[0][k] = S.c0[k];
            for (int j = 0; j < 3; ++j) {
                double u[3] = {U[o[j]], U[3 + o[j]], U[6 + o[j]]};
                int m = 0;   // the largest-magnitude component is positive, ties to the lowest index
                if (fabs(u[1]) > fabs(u[m])) m = 1;
                if (fabs(u[2]) > fabs(u[m])) m = 2;
                const double sg = u[m] < 0.0 ? -1.0 : 1.0;
                const double len = sqrt(fmax(w[o[j]], 0.0) / pn);
                for (int k = 0; k < 3; ++k) {
                    C[k * 3 + j] = len * (sg * u[k]);
                    S.cws[j + 1][k] = S.c0[k] + C[k * 3 + j];
                }
            }
            const double det = C[0] * (C[4] * C[8] - C[5] * C[7]) - C[1] * (C[3] * C[8] - C[5] * C[6]) +
                               C[2] * (C[3] * C[7] - C[4] * C[6]);
            S.ccinv[0][0] = (C[4] * C[8] - C[5] * C[7]) / det;
            S.ccinv[0][1] = (C[2] * C[7] - C[1] * C[8]) / det;
            S.ccinv[0][2] = (C[1] * C[5] - C[2] * C[4]) / det;
            S.ccinv[1][0] = (C[5] * C[6] - C[3] * C[8]) / det;
            S.ccinv[1][1] = (C[0] * C[8] - C[2] * C[6]) / det;
            S.ccinv[1][2] = (C[2] * C[3] - C[0] * C[5]) / det;
            S.ccinv[2][0] = (C[3] * C[7] - C[4] * C[6]) / det;
            S.ccinv[2][1] = (C[1] * C[6] - C[0] * C[7]) / det;
            S.ccinv[2][2] = (C[0] * C[4] - C[1] * C[3]) / det;
        }
    }
    if (S.degenerate) {
        PVE_PHASE(lane) {
            if (lane == 0) {
                degenerate_out(out);
                out.n_used = 1;
                out.cand_err[0] = out.cand_err[1] = out.cand_err[2] = NAN;
            }
        }
        return;
    }
    // ---- 2. barycentric coordinates
    PVE_PHASE(lane) {
        if (lane < pn) {
            const double d[3] = {S.pw[lane][0] - S.c0[0], S.pw[lane][1] - S.c0[1], S.pw[lane][2] - S.c0[2]};
            double sum = 0.0;
            for (int j = 0; j < 3; ++j) {
                const double a = S.ccinv[j][0] * d[0] + S.ccinv[j][1] * d[1] + S.ccinv[j][2] * d[2];
                S.al[lane][j + 1] = a;
                sum += a;
            }
            S.al[lane][0] = 1.0 - sum;
        }
    }
    // ---- 3. M^T M (78 unique entries over the lanes, points summed in index order), V = I
    PVE_PHASE(lane) {
        for (int e = lane; e < 78; e += kLanes) {
            int r = 0, rem = e;   // e -> (r, c), r <= c
            while (rem >= 12 - r) { rem -= 12 - r; ++r; }
            const int c = r + rem;
            double s = 0.0;
            for (int i = 0; i < pn; ++i) {
                double a1, a2, b1, b2;
                m_rows(S, i, r, &a1, &a2);
                m_rows(S, i, c, &b1, &b2);
                s += a1 * b1 + a2 * b2;
            }
            S.A[0][r * 12 + c] = s;
            S.A[0][c * 12 + r] = s;
        }
        for (int e = lane; e < 144; e += kLanes) S.V[0][e] = (e % 13 == 0) ? 1.0 : 0.0;
    }
    // cyclic Jacobi by round-robin steps: lanes 0..5 find the step's six disjoint rotations, then
    // every lane applies them to its entries of A and V.  A sweep without a rotation ends it.
    double trace = 0.0;
    for (int i = 0; i < 12; ++i) trace += fabs(S.A[0][i * 13]);
    const double tiny = kTiny * trace;
    int cur = 0;
    if (trace == trace && trace <= DBL_MAX) {   // a non-finite keypoint: nothing to iterate on
        for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
            for (int step = 0; step < 11; ++step) {
                PVE_PHASE(lane) {
                    if (lane < 6) {
                        int p, q;
                        jacobi_pair(step, lane, &p, &q);
                        const double apq = S.A[cur][p * 12 + q];
                        double c = 1.0, s = 0.0;
                        const int rot = fabs(apq) > tiny ? 1 : 0;
                        if (rot) {
                            const double th = (S.A[cur][q * 13] - S.A[cur][p * 13]) / (2.0 * apq);
                            const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                            c = 1.0 / sqrt(t * t + 1.0);
                            s = t * c;
                        }
                        S.jp[p] = q; S.jc[p] = c; S.js[p] = -s;
                        S.jp[q] = p; S.jc[q] = c; S.js[q] = s;
                        S.rot[lane] = rot;
                    }
                }
                PVE_PHASE(lane) {
                    const double *A = S.A[cur], *V = S.V[cur];
                    for (int e = lane; e < 144; e += kLanes) {
                        int i = e / 12, j = e - 12 * i;
                        const int pj = S.jp[j];
                        S.V[cur ^ 1][e] = S.jc[j] * V[i * 12 + j] + S.js[j] * V[i * 12 + pj];
                        if (i > j) { const int t = i; i = j; j = t; }   // (i, j) and (j, i) get the same bits
                        const int pi = S.jp[i], pjj = S.jp[j];
                        double a;
                        if (pi == j && S.js[i] != 0.0) {
                            a = 0.0;
                        } else {
                            const double x = S.jc[j] * A[i * 12 + j] + S.js[j] * A[i * 12 + pjj];
                            const double y = S.jc[j] * A[pi * 12 + j] + S.js[j] * A[pi * 12 + pjj];
                            a = S.jc[i] * x + S.js[i] * y;
                        }
                        S.A[cur ^ 1][e] = a;
                    }
                    if (lane == 0) {
                        int n = 0;
                        for (int k = 0; k < 6; ++k) n += S.rot[k];
                        S.nrot = step == 0 ? n : S.nrot + n;
                    }
                }
                cur ^= 1;
            }
            if (S.nrot == 0) break;
        }
    }
    // the four smallest eigenvalues, smallest first, ties to the lower index
    PVE_PHASE(lane) {
        if (lane == 0) {
            const double *A = S.A[cur];
            for (int k = 0; k < 4; ++k) {
                int best = -1;
                for (int i = 0; i < 12; ++i) {
                    bool taken = false;
                    for (int m = 0; m < k; ++m) taken = taken || S.vsel[m] == i;
                    if (!taken && (best < 0 || A[i * 13] < A[best * 13])) best = i;
                }
                S.vsel[k] = best;
            }
        }
    }
    PVE_PHASE(lane) {
        if (lane < 48) {
            const int k = lane / 12, i = lane - 12 * k;
            S.v[k][i] = S.V[cur][i * 12 + S.vsel[k]];
        }
    }
    // ---- 4. L [6][10] and rho [6], one control-point pair per lane
    PVE_PHASE(lane) {
        if (lane < 6) {
            const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
            const int a = pa[lane], b = pb[lane];
            double d[4][3], g[4][4];
            for (int k = 0; k < 4; ++k)
                for (int c = 0; c < 3; ++c) d[k][c] = S.v[k][3 * a + c] - S.v[k][3 * b + c];
            for (int k = 0; k < 4; ++k)
                for (int m = k; m < 4; ++m) g[k][m] = d[k][0] * d[m][0] + d[k][1] * d[m][1] + d[k][2] * d[m][2];
            double *l = S.L[lane];
            l[0] = g[0][0]; l[1] = 2.0 * g[0][1]; l[2] = g[1][1]; l[3] = 2.0 * g[0][2]; l[4] = 2.0 * g[1][2];
            l[5] = g[2][2]; l[6] = 2.0 * g[0][3]; l[7] = 2.0 * g[1][3]; l[8] = 2.0 * g[2][3]; l[9] = g[3][3];
            double r = 0.0;
            for (int c = 0; c < 3; ++c) r += (S.cws[a][c] - S.cws[b][c]) * (S.cws[a][c] - S.cws[b][c]);
            S.rho[lane] = r;
        }
    }
    // ---- 5, 6. the three beta starts and their Gauss-Newton, one candidate per lane; then the
    // candidate's control points in the camera frame, negated if point 0 lands behind the camera
    PVE_PHASE(lane) {
        if (lane < 3) {
            double be[4];
            solve_betas(S, lane, be);
            double cc[4][3], z0 = 0.0;
            for (int j = 0; j < 4; ++j) {
                for (int c = 0; c < 3; ++c)
                    cc[j][c] = be[0] * S.v[0][3 * j + c] + be[1] * S.v[1][3 * j + c] + be[2] * S.v[2][3 * j + c] +
                               be[3] * S.v[3][3 * j + c];
                z0 += S.al[0][j] * cc[j][2];
            }
            const double sg = z0 < 0.0 ? -1.0 : 1.0;
            for (int j = 0; j < 4; ++j)
                for (int c = 0; c < 3; ++c) S.ccs[lane][j][c] = sg * cc[j][c];
        }
    }
    // ---- 7. every candidate's points in the camera frame, Arun/Horn, reprojection error
    PVE_PHASE(lane) {
        if (lane < pn) {
            for (int n = 0; n < 3; ++n)
                for (int c = 0; c < 3; ++c) {
                    double s = 0.0;
                    for (int j = 0; j < 4; ++j) s += S.al[lane][j] * S.ccs[n][j][c];
                    S.pc[n][lane][c] = s;
                }
        }
    }
    PVE_PHASE(lane) {
        if (lane < 9) {
            const int n = lane / 3, c = lane - 3 * n;
            double s = 0.0;
            for (int i = 0; i < pn; ++i) s += S.pc[n][i][c];
            S.pc0[n][c] = s / pn;
        }
    }
    PVE_PHASE(lane) {
        if (lane < 27) {
            const int n = lane / 9, e = lane - 9 * n, j = e / 3, k = e - 3 * j;
            double s = 0.0;
            for (int i = 0; i < pn; ++i) s += (S.pc[n][i][j] - S.pc0[n][j]) * (S.pw[i][k] - S.c0[k]);
            S.abt[n][e] = s;
        }
    }
    PVE_PHASE(lane) {
        if (lane < 3) {
            double R[9];
            bool ok = true;
            for (int e = 0; e < 9; ++e) ok = ok && fabs(S.abt[lane][e]) <= DBL_MAX;
            S.bad[lane] = 0;
            if (!ok) {
                S.bad[lane] = 2;   // not finite: the error is NaN
                for (int e = 0; e < 9; ++e) R[e] = NAN;
            } else if (!polar_rotation3(S.abt[lane], R)) {
                S.bad[lane] = 1;   // no rotation: the error is +inf
                for (int e = 0; e < 9; ++e) R[e] = NAN;
            } else {
                const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                                   R[2] * (R[3] * R[7] - R[4] * R[6]);
                if (det < 0.0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            }
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) S.R[lane][r * 3 + c] = R[r * 3 + c];
                S.t[lane][r] = S.pc0[lane][r] - (R[r * 3] * S.c0[0] + R[r * 3 + 1] * S.c0[1] + R[r * 3 + 2] * S.c0[2]);
            }
        }
    }
    PVE_PHASE(lane) {
        if (lane < pn) {
            for (int n = 0; n < 3; ++n) {
                const double *R = S.R[n], *t = S.t[n], *p = S.pw[lane];
                const double X = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + t[0];
                const double Y = R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + t[1];
                const double Z = R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + t[2];
                // u - ue = (uc + fu X / Z) - u, with du = uc - u
                const double eu = S.du[lane] + S.cam[0] * X / Z, ev = S.dv[lane] + S.cam[1] * Y / Z;
                S.pc[n][lane][0] = sqrt(eu * eu + ev * ev);
            }
        }
    }
    PVE_PHASE(lane) {
        if (lane < 3) {
            double s = 0.0;
            for (int i = 0; i < pn; ++i) s += S.pc[lane][i][0];
            S.err[lane] = S.bad[lane] == 1 ? INFINITY : S.bad[lane] == 2 ? NAN : s / pn;
        }
    }
    // ---- 8, 9. cv2's strict choice; anything not finite becomes the degenerate answer
    PVE_PHASE(lane) {
        if (lane == 0) {
            int n = 0;
            if (S.err[1] < S.err[0]) n = 1;
            if (S.err[2] < S.err[n]) n = 2;
            out.n_used = n + 1;
            for (int k = 0; k < 3; ++k) out.cand_err[k] = S.err[k];
            bool ok = fabs(S.err[n]) <= DBL_MAX;
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) {
                    out.Rt[r * 4 + c] = S.R[n][r * 3 + c];
                    ok = ok && fabs(S.R[n][r * 3 + c]) <= DBL_MAX;
                }
                out.Rt[r * 4 + 3] = S.t[n][r];
                out.rt6[3 + r] = S.t[n][r];
                ok = ok && fabs(S.t[n][r]) <= DBL_MAX;
            }
            if (ok) {
                rodrigues_to_vec(S.R[n], out.rt6);
                ok = fabs(out.rt6[0]) <= DBL_MAX && fabs(out.rt6[1]) <= DBL_MAX && fabs(out.rt6[2]) <= DBL_MAX;
            }
            out.status = kStatusOk;
            if (!ok) degenerate_out(out);
        }
    }
}

}  // namespace pve
