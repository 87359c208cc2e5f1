// Pose-graph optimisation of the loop-closing 360 merge (Old/new360Merge.py:
// 121-131: global_optimization(pose_graph, GlobalOptimizationLevenbergMarquardt(),
// GlobalOptimizationConvergenceCriteria(), GlobalOptimizationOption(0.4 voxel,
// 0.25, reference_node 0))).  Plain host C++: no GPU call, so it runs and is
// tested on a machine without one.  Open3D's algorithm restated (parity with
// Open3D is unpinned: not in this image); tests/posegraph_oracle.py restates
// this exact arithmetic and DESIGN.md 5.7 gives the contract.  Every edge is
// certain: the line process and edge pruning are not implemented.
//
//   vec6(M)   sy = sqrt(R00^2 + R10^2); sy >= 1e-6: (atan2(R21, R22),
//             atan2(-R20, sy), atan2(R10, R00)), else (atan2(-R12, R11),
//             atan2(-R20, sy), 0); then the translation.
//   mat(v)    R = Rz(v2) (Ry(v1) Rx(v0)), translation v3..5.
//   edge      e = vec6((X^-1 T_t^-1) T_s); column a of J_s = lin6(((X^-1
//             T_t^-1) G_a) T_s), of J_t the same with -G_a; lin6(M) =
//             ((M21 - M12) / 2, (M02 - M20) / 2, (M10 - M01) / 2, M03, M13, M23).
//   system    dense 6N x 6N: H += J^T L J (four blocks per edge, edges in list
//             order), b -= J^T L e, residual += e^T L e; the reference node's
//             rows and columns zeroed, diagonal 1, b 0.
//   LM        lambda = 1e-5 max diag H, nu = 2; (H + lambda I) delta = b by
//             LDL^T without pivoting; T_i <- mat(delta_i) T_i; rho = (r - r_new)
//             / (delta . (lambda delta + b) + 1e-3); rho > 0: accept, lambda *=
//             max(1/3, 1 - (2 rho - 1)^3), nu = 2; else lambda *= nu, nu *= 2,
//             at most max_iteration_lm tries.  A step whose delta is not finite
//             counts as rejected.
// Products of 4x4 matrices in icp_mat4's order, sums of products as left folds
// from 0.0; inverses are rigid inverses, -((R0i t0 + R1i t1) + R2i t2).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace pg {

struct M4 {
  double m[16];
};

inline M4 mul(const M4& a, const M4& b) {
  M4 o;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      o.m[4 * i + j] = ((a.m[4 * i] * b.m[j] + a.m[4 * i + 1] * b.m[4 + j]) + a.m[4 * i + 2] * b.m[8 + j]) +
                       a.m[4 * i + 3] * b.m[12 + j];
  return o;
}

inline M4 rigid_inverse(const M4& a) {
  M4 o;
  memset(o.m, 0, sizeof(o.m));
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.m[4 * i + j] = a.m[4 * j + i];
    o.m[4 * i + 3] = -((a.m[i] * a.m[3] + a.m[4 + i] * a.m[7]) + a.m[8 + i] * a.m[11]);
  }
  o.m[15] = 1.0;
  return o;
}

inline void vec6(const M4& M, double* v) {
  const double* m = M.m;
  const double sy = sqrt(m[0] * m[0] + m[4] * m[4]);
  if (sy >= 1e-6) {
    v[0] = atan2(m[9], m[10]);
    v[1] = atan2(-m[8], sy);
    v[2] = atan2(m[4], m[0]);
  } else {
    v[0] = atan2(-m[6], m[5]);
    v[1] = atan2(-m[8], sy);
    v[2] = 0.0;
  }
  v[3] = m[3];
  v[4] = m[7];
  v[5] = m[11];
}

inline void mul3(const double a[3][3], const double b[3][3], double o[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o[i][j] = (a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j];
}

inline M4 mat(const double* v) {
  const double ca = cos(v[0]), sa = sin(v[0]), cb = cos(v[1]), sb = sin(v[1]), cg = cos(v[2]), sg = sin(v[2]);
  const double Rx[3][3] = {{1.0, 0.0, 0.0}, {0.0, ca, -sa}, {0.0, sa, ca}};
  const double Ry[3][3] = {{cb, 0.0, sb}, {0.0, 1.0, 0.0}, {-sb, 0.0, cb}};
  const double Rz[3][3] = {{cg, -sg, 0.0}, {sg, cg, 0.0}, {0.0, 0.0, 1.0}};
  double T[3][3], R[3][3];
  mul3(Ry, Rx, T);
  mul3(Rz, T, R);
  M4 o;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.m[4 * i + j] = R[i][j];
    o.m[4 * i + 3] = v[3 + i];
  }
  o.m[12] = o.m[13] = o.m[14] = 0.0;
  o.m[15] = 1.0;
  return o;
}

inline void lin6(const M4& M, double* v) {
  const double* m = M.m;
  v[0] = (m[9] - m[6]) / 2.0;
  v[1] = (m[2] - m[8]) / 2.0;
  v[2] = (m[4] - m[1]) / 2.0;
  v[3] = m[3];
  v[4] = m[7];
  v[5] = m[11];
}

// generator a (rotations about x, y, z, then translations) times sign
inline M4 generator(int a, double sign) {
  M4 g;
  memset(g.m, 0, sizeof(g.m));
  if (a < 3) {
    static const int at[3][2] = {{2, 1}, {0, 2}, {1, 0}};
    g.m[4 * at[a][0] + at[a][1]] = sign;
    g.m[4 * at[a][1] + at[a][0]] = -sign;
  } else {
    g.m[4 * (a - 3) + 3] = sign;
  }
  return g;
}

inline double dot(const double* u, const double* v, int n, int su = 1, int sv = 1) {
  double s = 0.0;
  for (int k = 0; k < n; ++k) s = s + u[k * su] * v[k * sv];
  return s;
}

struct Edge {
  int s, t;
  M4 X;
  const double* L;  // information, 6x6 row-major
};

// e^T L e of one edge (and e)
inline double edge_residual(const M4& Ts, const M4& Tt, const Edge& E, M4* A_out, double* e) {
  const M4 A = mul(rigid_inverse(E.X), rigid_inverse(Tt));
  vec6(mul(A, Ts), e);
  double Le[6];
  for (int m = 0; m < 6; ++m) Le[m] = dot(E.L + 6 * m, e, 6);
  if (A_out) *A_out = A;
  return dot(e, Le, 6);
}

inline double graph_residual(const std::vector<M4>& T, const std::vector<Edge>& edges) {
  double r = 0.0, e[6];
  for (const Edge& E : edges) r = r + edge_residual(T[E.s], T[E.t], E, nullptr, e);
  return r;
}

// H (n6 x n6, row-major), b and the residual at poses T
inline double linearise(const std::vector<M4>& T, const std::vector<Edge>& edges, int ref, std::vector<double>& H,
                        std::vector<double>& b) {
  const size_t n6 = 6 * T.size();
  std::fill(H.begin(), H.end(), 0.0);
  std::fill(b.begin(), b.end(), 0.0);
  double r = 0.0;
  for (const Edge& E : edges) {
    M4 A;
    double e[6], J[2][36], W[2][36], col[6];
    r = r + edge_residual(T[E.s], T[E.t], E, &A, e);
    for (int a = 0; a < 6; ++a)
      for (int side = 0; side < 2; ++side) {
        lin6(mul(mul(A, generator(a, side ? -1.0 : 1.0)), T[E.s]), col);
        for (int m = 0; m < 6; ++m) J[side][6 * m + a] = col[m];
      }
    for (int side = 0; side < 2; ++side)  // W = J^T L
      for (int a = 0; a < 6; ++a)
        for (int k = 0; k < 6; ++k) W[side][6 * a + k] = dot(J[side] + a, E.L + k, 6, 6, 6);
    const int id[2] = {E.s, E.t};
    for (int p = 0; p < 2; ++p) {
      for (int q = 0; q < 2; ++q)
        for (int a = 0; a < 6; ++a)
          for (int c = 0; c < 6; ++c) {
            double& h = H[(6 * static_cast<size_t>(id[p]) + a) * n6 + 6 * static_cast<size_t>(id[q]) + c];
            h = h + dot(W[p] + 6 * a, J[q] + c, 6, 1, 6);
          }
      for (int a = 0; a < 6; ++a) {
        double& v = b[6 * static_cast<size_t>(id[p]) + a];
        v = v - dot(W[p] + 6 * a, e, 6);
      }
    }
  }
  for (size_t a = 6 * static_cast<size_t>(ref); a < 6 * static_cast<size_t>(ref) + 6; ++a) {
    for (size_t k = 0; k < n6; ++k) H[a * n6 + k] = H[k * n6 + a] = 0.0;
    H[a * n6 + a] = 1.0;
    b[a] = 0.0;
  }
  return r;
}

// x of A x = b by A = L D L^T without pivoting (A: n x n row-major; L is scratch
// of the same size); a zero pivot gives NaN
inline void ldlt_solve(const std::vector<double>& A, const std::vector<double>& b, size_t n, std::vector<double>& L,
                       std::vector<double>& d, std::vector<double>& x) {
  for (size_t j = 0; j < n; ++j) {
    double v = 0.0;
    for (size_t q = 0; q < j; ++q) v = v + (L[j * n + q] * d[q]) * L[j * n + q];
    d[j] = A[j * n + j] - v;
    for (size_t i = j + 1; i < n; ++i) {
      double w = 0.0;
      for (size_t q = 0; q < j; ++q) w = w + (L[i * n + q] * d[q]) * L[j * n + q];
      L[i * n + j] = d[j] != 0.0 ? (A[i * n + j] - w) / d[j] : NAN;
    }
  }
  x = b;
  for (size_t i = 0; i < n; ++i) {
    double v = 0.0;
    for (size_t q = 0; q < i; ++q) v = v + L[i * n + q] * x[q];
    x[i] = x[i] - v;
  }
  for (size_t i = 0; i < n; ++i) x[i] = d[i] != 0.0 ? x[i] / d[i] : NAN;
  for (size_t i = n; i-- > 0;) {
    double v = 0.0;
    for (size_t q = i + 1; q < n; ++q) v = v + L[q * n + i] * x[q];
    x[i] = x[i] - v;
  }
}

inline double max_abs(const std::vector<double>& v) {
  double m = 0.0;
  for (double x : v) m = fabs(x) > m ? fabs(x) : m;
  return m;
}

}  // namespace pg

extern "C" int sl_pose_graph_optimize(double* poses, int n_nodes, const int32_t* edge_source,
                                      const int32_t* edge_target, const double* edge_transformation,
                                      const double* edge_information, const uint8_t* edge_uncertain, int n_edges,
                                      int reference_node, int max_iteration, int max_iteration_lm,
                                      double min_right_term, double min_relative_increment,
                                      double min_relative_residual_increment, double min_residual, int* iterations,
                                      double* initial_residual, double* final_residual) {
  using namespace pg;
  if (!poses || n_nodes <= 0 || n_edges < 0 || reference_node < 0 || reference_node >= n_nodes ||
      max_iteration < 0 || max_iteration_lm < 1 ||
      (n_edges && (!edge_source || !edge_target || !edge_transformation || !edge_information)))
    return SL_EINVAL;
  for (int k = 0; k < n_edges; ++k)
    if (edge_source[k] < 0 || edge_source[k] >= n_nodes || edge_target[k] < 0 || edge_target[k] >= n_nodes ||
        (edge_uncertain && edge_uncertain[k]))  // uncertain edges need the line process: not implemented
      return SL_EINVAL;
  std::vector<M4> T(static_cast<size_t>(n_nodes)), cand(static_cast<size_t>(n_nodes));
  memcpy(T.data(), poses, sizeof(M4) * T.size());
  std::vector<Edge> edges(static_cast<size_t>(n_edges));
  for (int k = 0; k < n_edges; ++k) {
    edges[k].s = edge_source[k];
    edges[k].t = edge_target[k];
    memcpy(edges[k].X.m, edge_transformation + 16 * static_cast<size_t>(k), sizeof(M4));
    edges[k].L = edge_information + 36 * static_cast<size_t>(k);
  }
  const size_t n6 = 6 * T.size();
  std::vector<double> H(n6 * n6), Hl(n6 * n6), L(n6 * n6, 0.0), b(n6), d(n6), delta(n6), x(n6);
  double r = linearise(T, edges, reference_node, H, b);
  const double r0 = r;
  double lam = 0.0, nu = 2.0;
  for (size_t k = 0; k < n6; ++k) lam = H[k * n6 + k] > lam ? H[k * n6 + k] : lam;
  lam = 1e-5 * lam;
  bool stop = max_abs(b) < min_right_term || r < min_residual;
  int it = 0;
  while (it < max_iteration && !stop) {
    int tries = 0;
    for (;;) {
      Hl = H;
      for (size_t k = 0; k < n6; ++k) Hl[k * n6 + k] = Hl[k * n6 + k] + lam;
      ldlt_solve(Hl, b, n6, L, d, delta);
      bool finite = true;
      for (double v : delta) finite = finite && std::isfinite(v);
      double rho = -1.0, r_new = 0.0;
      if (finite) {
        for (size_t i = 0; i < T.size(); ++i) vec6(T[i], &x[6 * i]);
        if (sqrt(dot(delta.data(), delta.data(), static_cast<int>(n6))) <
            min_relative_increment * (sqrt(dot(x.data(), x.data(), static_cast<int>(n6))) + min_relative_increment)) {
          stop = true;
          break;
        }
        for (size_t i = 0; i < T.size(); ++i) cand[i] = mul(mat(&delta[6 * i]), T[i]);
        r_new = graph_residual(cand, edges);
        for (size_t k = 0; k < n6; ++k) x[k] = lam * delta[k] + b[k];
        rho = (r - r_new) / (dot(delta.data(), x.data(), static_cast<int>(n6)) + 1e-3);
      }
      if (rho > 0.0) {
        if (fabs(r - r_new) < min_relative_residual_increment * r) stop = true;
        T = cand;
        r = linearise(T, edges, reference_node, H, b);
        if (max_abs(b) < min_right_term) stop = true;
        const double t = 2.0 * rho - 1.0;
        const double f = 1.0 - (t * t) * t;
        lam = lam * (f > 1.0 / 3.0 ? f : 1.0 / 3.0);
        nu = 2.0;
      } else {
        lam = lam * nu;
        nu = 2.0 * nu;
      }
      ++tries;
      if (rho > 0.0 || tries >= max_iteration_lm || stop) break;
    }
    ++it;
    if (r < min_residual) stop = true;
  }
  memcpy(poses, T.data(), sizeof(M4) * T.size());
  if (iterations) *iterations = it;
  if (initial_residual) *initial_residual = r0;
  if (final_residual) *final_residual = r;
  return SL_OK;
}
