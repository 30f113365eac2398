// lk_expm.h -- dense matrix exponential on the HOST (lk_expm_dense): what stdlib_linalg's `expm` is to the reference's
// kexpm (src/Expm/ExpmLib.fypp:12, 207) -- and, at the end, the spectral norm of a small matrix (lk_norm2_dense, :346).  Plain C++: no device, no context, no LAPACK.  Included by lk_engine.hip; a stand-alone
// host program may include it too (it needs nothing but the public header).
//
// Scaling and squaring with the [13/13] Pade approximant (N. J. Higham, "The scaling and squaring method for the matrix
// exponential revisited", SIAM J. Matrix Anal. Appl. 26 (2005), algorithm 2.3 without the lower degrees): s = the smallest
// integer >= 0 with ||A / 2^s||_1 <= theta_13, r_13 = (V - U)^-1 (V + U) with U odd / V even in A from A^2, A^4, A^6 (six
// products), the linear system by an LU factorisation with partial pivoting written below, then s squarings.
#pragma once
#include "../../include/lightkrylov_hip.h"

#include <cmath>
#include <complex>
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

namespace lk_expm {

constexpr double THETA13 = 5.371920351148152;
constexpr double PADE13[14] = {64764752532480000.0, 32382376266240000.0, 7771770303897600.0, 1187353796428800.0, 129060195264000.0,
                               10559470521600.0,    670442572800.0,      33522128640.0,      1323241920.0,       40840800.0,
                               960960.0,            16380.0,             182.0,              1.0};

inline double abs1(double v) { return std::fabs(v); }
inline double abs1(const std::complex<double> &v) { return std::hypot(v.real(), v.imag()); }

// C = A B, n x n, column-major and packed (leading dimension n); C must not alias A or B
template <typename T>
void matmul(int n, const T *A, const T *B, T *C) {
    for (int j = 0; j < n; ++j) {
        T *c = C + (size_t)j * n;
        for (int i = 0; i < n; ++i) c[i] = T(0);
        for (int k = 0; k < n; ++k) {
            const T b = B[(size_t)j * n + k];
            if (b == T(0)) continue;
            const T *a = A + (size_t)k * n;
            for (int i = 0; i < n; ++i) c[i] += a[i] * b;
        }
    }
}

// X <- M^-1 X by LU with partial pivoting (M is overwritten by its factors); false when a pivot is exactly zero
template <typename T>
bool lu_solve(int n, T *M, T *X) {
    for (int k = 0; k < n; ++k) {
        int p = k;
        double big = abs1(M[(size_t)k * n + k]);
        for (int i = k + 1; i < n; ++i) {
            const double v = abs1(M[(size_t)k * n + i]);
            if (v > big) { big = v; p = i; }
        }
        if (!(big > 0.0)) return false;
        if (p != k) {
            for (int j = 0; j < n; ++j) {
                std::swap(M[(size_t)j * n + k], M[(size_t)j * n + p]);
                std::swap(X[(size_t)j * n + k], X[(size_t)j * n + p]);
            }
        }
        const T piv = M[(size_t)k * n + k];
        for (int i = k + 1; i < n; ++i) M[(size_t)k * n + i] /= piv;
        for (int j = k + 1; j < n; ++j) {
            const T f = M[(size_t)j * n + k];
            if (f == T(0)) continue;
            const T *l = M + (size_t)k * n;
            T *m = M + (size_t)j * n;
            for (int i = k + 1; i < n; ++i) m[i] -= l[i] * f;
        }
    }
    for (int j = 0; j < n; ++j) {
        T *x = X + (size_t)j * n;
        for (int k = 0; k < n; ++k) {                          // L y = P x (unit lower)
            const T f = x[k];
            if (f == T(0)) continue;
            const T *l = M + (size_t)k * n;
            for (int i = k + 1; i < n; ++i) x[i] -= l[i] * f;
        }
        for (int k = n - 1; k >= 0; --k) {                     // U z = y
            x[k] /= M[(size_t)k * n + k];
            const T f = x[k];
            const T *u = M + (size_t)k * n;
            for (int i = 0; i < k; ++i) x[i] -= u[i] * f;
        }
    }
    return true;
}

// E = exp(A): A (leading dimension lda) and E (lde) n x n column-major; E may be A itself.  A matrix with a non-finite entry gives
// an E of NaNs (as the approximant itself would), never a loop without end.
template <typename T>
void expm(int n, const T *A, int64_t lda, T *E, int64_t lde) {
    const size_t nn = (size_t)n * n;
    std::vector<T> buf(6 * nn);
    T *As = buf.data(), *A2 = As + nn, *A4 = A2 + nn, *A6 = A4 + nn, *U = A6 + nn, *V = U + nn;
    double norm1 = 0.0;
    bool finite = true;
    for (int j = 0; j < n; ++j) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) {
            const T v = A[(size_t)j * lda + i];
            As[(size_t)j * n + i] = v;
            s += abs1(v);
        }
        if (!std::isfinite(s)) finite = false;
        if (s > norm1) norm1 = s;
    }
    if (!finite) {
        const double q = std::numeric_limits<double>::quiet_NaN();
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) E[(size_t)j * lde + i] = T(q);
        return;
    }
    int s = 0;
    if (norm1 > THETA13) {
        int e = 0;
        (void)std::frexp(norm1 / THETA13, &e);               // norm1 / theta = f 2^e, 0.5 <= f < 1: 2^e >= the ratio
        s = e;
        const double sc = std::ldexp(1.0, -s);
        for (size_t i = 0; i < nn; ++i) As[i] *= sc;
    }
    const double *b = PADE13;
    matmul(n, As, As, A2);
    matmul(n, A2, A2, A4);
    matmul(n, A4, A2, A6);
    // U = A [A6 (b13 A6 + b11 A4 + b9 A2) + b7 A6 + b5 A4 + b3 A2 + b1 I],  V = A6 (b12 A6 + b10 A4 + b8 A2) + b6 A6 + b4 A4 + b2 A2 + b0 I
    std::vector<T> wbuf(2 * nn);
    T *W = wbuf.data(), *Z = W + nn;
    for (size_t i = 0; i < nn; ++i) W[i] = b[13] * A6[i] + b[11] * A4[i] + b[9] * A2[i];
    matmul(n, A6, W, Z);
    for (size_t i = 0; i < nn; ++i) Z[i] += b[7] * A6[i] + b[5] * A4[i] + b[3] * A2[i];
    for (int i = 0; i < n; ++i) Z[(size_t)i * n + i] += b[1];
    matmul(n, As, Z, U);
    for (size_t i = 0; i < nn; ++i) W[i] = b[12] * A6[i] + b[10] * A4[i] + b[8] * A2[i];
    matmul(n, A6, W, V);
    for (size_t i = 0; i < nn; ++i) V[i] += b[6] * A6[i] + b[4] * A4[i] + b[2] * A2[i];
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] += b[0];
    for (size_t i = 0; i < nn; ++i) {                          // W = V - U (factorised), Z = V + U (right-hand sides, then r_13)
        W[i] = V[i] - U[i];
        Z[i] = V[i] + U[i];
    }
    if (!lu_solve(n, W, Z)) {                                  // cannot happen for ||A|| <= theta_13 (V - U is well conditioned there)
        const double q = std::numeric_limits<double>::quiet_NaN();
        for (size_t i = 0; i < nn; ++i) Z[i] = T(q);
    }
    T *R = Z, *S = W;
    for (int t = 0; t < s; ++t) {
        matmul(n, R, R, S);
        std::swap(R, S);
    }
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) E[(size_t)j * lde + i] = R[(size_t)j * n + i];
}

// ||A||_2, the largest singular value of an m x n column-major matrix (leading dimension lda): what `norm(., 2)` is to kexpm_mat's
// error estimate (ExpmLib.fypp:346).  One-sided Jacobi (Hestenes): plane rotations from the right make the columns of a packed copy
// mutually orthogonal -- for the pair (p, q) with a = ||g_p||^2, b = ||g_q||^2, g = g_p^H g_q = |g| w: zeta = (b - a) / (2 |g|),
// t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = c t, g_p <- c g_p - s conj(w) g_q, g_q <- s w g_p + c g_q --
// until a whole sweep finds every pair orthogonal to machine precision; the singular values are then the column norms.  A wide matrix
// is handled through its conjugate transpose (min(m, n) columns).  Small singular values come out to high RELATIVE accuracy, which a
// route through A^H A would lose.  A non-finite entry gives NaN or Inf, never a loop without end (the sweeps are bounded).
inline double conj1(double v) { return v; }
inline std::complex<double> conj1(const std::complex<double> &v) { return std::conj(v); }
inline double real1(double v) { return v; }
inline double real1(const std::complex<double> &v) { return v.real(); }

template <typename T>
double norm2(int m, int n, const T *A, int64_t lda) {
    if (m <= 0 || n <= 0) return 0.0;
    const bool wide = n > m;
    const int rows = wide ? n : m, cols = wide ? m : n;
    std::vector<T> G((size_t)rows * cols);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) {
            const T v = A[(size_t)j * lda + i];
            if (wide) G[(size_t)i * rows + j] = conj1(v);
            else G[(size_t)j * rows + i] = v;
        }
    const double eps = std::numeric_limits<double>::epsilon();
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p + 1 < cols; ++p)
            for (int q = p + 1; q < cols; ++q) {
                T *gp = G.data() + (size_t)p * rows, *gq = G.data() + (size_t)q * rows;
                double a = 0.0, b = 0.0;
                T g = T(0);
                for (int i = 0; i < rows; ++i) {
                    a += real1(conj1(gp[i]) * gp[i]);
                    b += real1(conj1(gq[i]) * gq[i]);
                    g += conj1(gp[i]) * gq[i];
                }
                const double ag = abs1(g);
                if (!(ag > eps * std::sqrt(a) * std::sqrt(b))) continue;          // orthogonal already (or not a number: left alone)
                rotated = true;
                const T w = g / ag;
                const double zeta = (b - a) / (2.0 * ag);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                const T sw = s * w, swc = s * conj1(w);
                for (int i = 0; i < rows; ++i) {
                    const T u = gp[i], v = gq[i];
                    gp[i] = c * u - swc * v;
                    gq[i] = sw * u + c * v;
                }
            }
        if (!rotated) break;
    }
    double best = 0.0;
    bool anynan = false;
    for (int j = 0; j < cols; ++j) {
        const T *gj = G.data() + (size_t)j * rows;
        double scale = 0.0;
        for (int i = 0; i < rows; ++i) scale = std::fmax(scale, abs1(gj[i]));     // (fmax ignores a NaN: looked for below)
        double s = 0.0;
        bool nan = false;
        for (int i = 0; i < rows; ++i) {
            const double v = abs1(gj[i]);
            if (v != v) nan = true;
            if (scale > 0.0 && std::isfinite(scale)) s += (v / scale) * (v / scale);
        }
        double nj = (scale > 0.0 && std::isfinite(scale)) ? scale * std::sqrt(s) : scale;
        if (nan) anynan = true;
        if (nj > best) best = nj;
    }
    if (anynan) return std::numeric_limits<double>::quiet_NaN();
    return best;
}

}  // namespace lk_expm
