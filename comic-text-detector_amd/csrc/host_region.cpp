// The pixel-free part of `TextBlock.get_transformed_region` (reference utils/textblock.py:162-194) for n text lines in one
// call: margin, edge-midpoint ratio, crop size, the four-point homography and its inverse.  Plain float64 in the reference's
// operation order, compiled without contraction (Makefile host rule), so the crop sizes -- which hang on a round-half-even of
// textheight / ratio -- are the bits numpy gives.  What cv2 contributes there is restated from the published algorithm
// (parity unpinned): cv2.findHomography on exactly four points returns the unique homography through them
// normalised to h22 = 1; it is solved here as cv2.getPerspectiveTransform solves it (8x8 system, LU with partial
// pivoting); cv2.warpPerspective inverts it by the adjugate formula (cv::invert, 3x3 double).
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ctd_hip.h"

namespace {

// cv::solve(DECOMP_LU) of the 8x8 system: Gaussian elimination with partial pivoting, a pivot below 100 eps is singular
bool solve8(double A[8][8], double b[8]) {
  const int n = 8;
  for (int i = 0; i < n; ++i) {
    int k = i;
    for (int j = i + 1; j < n; ++j)
      if (std::fabs(A[j][i]) > std::fabs(A[k][i])) k = j;
    if (!(std::fabs(A[k][i]) >= 2.220446049250313e-16 * 100)) return false;   // also rejects a nan pivot
    if (k != i) {
      for (int j = i; j < n; ++j) {
        const double t = A[i][j];
        A[i][j] = A[k][j];
        A[k][j] = t;
      }
      const double t = b[i];
      b[i] = b[k];
      b[k] = t;
    }
    const double d = -1 / A[i][i];
    for (int j = i + 1; j < n; ++j) {
      const double alpha = A[j][i] * d;
      for (int c = i + 1; c < n; ++c) A[j][c] += alpha * A[i][c];
      b[j] += alpha * b[i];
    }
  }
  for (int i = n - 1; i >= 0; --i) {
    double s = b[i];
    for (int c = i + 1; c < n; ++c) s -= A[i][c] * b[c];
    b[i] = s / A[i][i];
  }
  return true;
}

// cv::invert of a 3x3 double matrix: adjugate times 1 / det
bool invert3(const double* S, double* D) {
  const double det = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
  if (det == 0 || !std::isfinite(det)) return false;
  const double d = 1. / det;
  D[0] = (S[4] * S[8] - S[5] * S[7]) * d;
  D[1] = (S[2] * S[7] - S[1] * S[8]) * d;
  D[2] = (S[1] * S[5] - S[2] * S[4]) * d;
  D[3] = (S[5] * S[6] - S[3] * S[8]) * d;
  D[4] = (S[0] * S[8] - S[2] * S[6]) * d;
  D[5] = (S[2] * S[3] - S[0] * S[5]) * d;
  D[6] = (S[3] * S[7] - S[4] * S[6]) * d;
  D[7] = (S[1] * S[6] - S[0] * S[7]) * d;
  D[8] = (S[0] * S[4] - S[1] * S[3]) * d;
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(D[i])) return false;
  return true;
}

constexpr double REGION_RESIDUAL_MAX = 1e-4;   // pixels of the crop; a well-posed quad leaves ~1e-9

inline double clip(double v, double lo, double hi) { return std::fmin(std::fmax(v, lo), hi); }   // np.clip

// int(round(v)) of a finite double within the side limit, else 0
int32_t round_side(double v) {
  if (!std::isfinite(v)) return 0;
  const double r = std::nearbyint(v);   // half-even in the default rounding mode, like Python's round
  return (r >= 1 && r <= CTD_REGION_MAX_SIDE) ? (int32_t)r : 0;
}

bool one_line(const int32_t* q, int language, bool vertical, double font_size, int im_w, int im_h, double textheight,
              int32_t* wh, double* M, double* Minv) {
  double x[4], y[4];
  for (int i = 0; i < 4; ++i) {
    x[i] = (double)q[2 * i];
    y[i] = (double)q[2 * i + 1];
  }
  if (language == 0 || (language == 2 && !vertical)) {   // textblock.py:167-172
    const double e = font_size / 3;
    const double sx[4] = {-e, e, e, -e}, sy[4] = {-e, -e, e, e};
    for (int i = 0; i < 4; ++i) {
      x[i] = clip(x[i] + sx[i], 0, (double)im_w);
      y[i] = clip(y[i] + sy[i], 0, (double)im_h);
    }
  }
  double mx[4], my[4];                                   // :174 midpoints of edges 0-1, 1-2, 2-3, 3-0
  for (int i = 0; i < 4; ++i) {
    mx[i] = (x[(i + 1) & 3] + x[i]) / 2;
    my[i] = (y[(i + 1) & 3] + y[i]) / 2;
  }
  const double vx = mx[2] - mx[0], vy = my[2] - my[0], hx = mx[1] - mx[3], hy = my[1] - my[3];
  const double ratio = std::sqrt(vx * vx + vy * vy) / std::sqrt(hx * hx + hy * hy);
  if (!std::isfinite(textheight) || !(textheight >= 1 && textheight <= CTD_REGION_MAX_SIDE)) return false;
  int32_t w, h;
  if (!vertical) {
    h = (int32_t)textheight;                             // int(textheight) truncates
    w = round_side(textheight / ratio);
  } else {
    w = (int32_t)textheight;
    h = round_side(textheight * ratio);
  }
  if (w < 1 || h < 1) return false;
  const double u[4] = {0, (double)(w - 1), (double)(w - 1), 0}, v[4] = {0, 0, (double)(h - 1), (double)(h - 1)};
  double A[8][8], b[8];
  for (int i = 0; i < 4; ++i) {
    const double ra[8] = {x[i], y[i], 1, 0, 0, 0, -x[i] * u[i], -y[i] * u[i]};
    const double rb[8] = {0, 0, 0, x[i], y[i], 1, -x[i] * v[i], -y[i] * v[i]};
    for (int c = 0; c < 8; ++c) {
      A[i][c] = ra[c];
      A[i + 4][c] = rb[c];
    }
    b[i] = u[i];
    b[i + 4] = v[i];
  }
  if (!solve8(A, b)) return false;
  for (int i = 0; i < 8; ++i) {
    if (!std::isfinite(b[i])) return false;
    M[i] = b[i];
  }
  M[8] = 1.;
  // collinear source points have no homography onto a rectangle, yet rounding may leave the elimination a tiny non-zero
  // pivot and a finite, meaningless solution: what was solved must map the four points where they belong
  for (int i = 0; i < 4; ++i) {
    const double den = (M[6] * x[i] + M[7] * y[i]) + M[8];
    const double px = ((M[0] * x[i] + M[1] * y[i]) + M[2]) / den, py = ((M[3] * x[i] + M[4] * y[i]) + M[5]) / den;
    if (!(std::fabs(px - u[i]) <= REGION_RESIDUAL_MAX && std::fabs(py - v[i]) <= REGION_RESIDUAL_MAX)) return false;
  }
  if (!invert3(M, Minv)) return false;
  wh[0] = w;
  wh[1] = h;
  return true;
}

}  // namespace

extern "C" int ctd_region_transforms(const int32_t* quads, const int32_t* language, const int32_t* vertical,
                                     const double* font_size, const int32_t* im_w, const int32_t* im_h, int32_t n,
                                     double textheight, int32_t* wh, double* M, double* Minv, int32_t* status) {
  if (n < 0) return CTD_ERR_INVALID;
  if (n > 0 && (!quads || !language || !vertical || !font_size || !im_w || !im_h || !wh || !M || !Minv || !status))
    return CTD_ERR_INVALID;
  for (int32_t i = 0; i < n; ++i) {
    double m[9] = {0}, mi[9] = {0};
    int32_t s[2] = {0, 0};
    const bool ok = one_line(quads + 8 * (size_t)i, language[i], vertical[i] != 0, font_size[i], im_w[i], im_h[i], textheight,
                             s, m, mi);
    for (int k = 0; k < 9; ++k) {
      M[9 * (size_t)i + k] = ok ? m[k] : 0.;
      Minv[9 * (size_t)i + k] = ok ? mi[k] : 0.;
    }
    wh[2 * (size_t)i] = ok ? s[0] : 0;
    wh[2 * (size_t)i + 1] = ok ? s[1] : 0;
    status[i] = ok ? CTD_REGION_OK : CTD_REGION_DEGENERATE;
  }
  return CTD_OK;
}
