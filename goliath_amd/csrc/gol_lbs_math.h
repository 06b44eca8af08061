// gol_lbs_math.h -- the per-joint algebra of the skeleton solve (csrc/lbs.hip) and its derivatives, in double.
//
// Quaternions are xyzw and are NOT assumed to be unit: every function is the derivative of the reference's polynomial
// (ca_code/utils/quaternion.py), not of a rotation.  Plain functions of values, usable from host code as well:
// tests/lbs_math_fd.cpp compiles this header for the host and checks every derivative against central differences.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define GOL_HD __host__ __device__ __forceinline__
#else
#define GOL_HD inline
#endif

namespace gol_lbs {

struct D3 {
  double x, y, z;
};
struct Q4 {
  double x, y, z, w;
};
// a joint's state (lbs.py:347-349): translation, rotation, scale
struct State {
  D3 t;
  Q4 q;
  double s;
};

GOL_HD D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
GOL_HD D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
GOL_HD double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
GOL_HD D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
GOL_HD Q4 operator+(Q4 a, Q4 b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

// Quaternion.batchMul (quaternion.py:178-249)
GOL_HD Q4 qmul(Q4 q, Q4 r) {
  return {q.x * r.w + q.y * r.z - q.z * r.y + q.w * r.x, -q.x * r.z + q.y * r.w + q.z * r.x + q.w * r.y,
          q.x * r.y - q.y * r.x + q.z * r.w + q.w * r.z, -q.x * r.x - q.y * r.y - q.z * r.z + q.w * r.w};
}
GOL_HD Q4 qmul_bwd_q(Q4 r, Q4 g) {
  return {g.x * r.w - g.y * r.z + g.z * r.y - g.w * r.x, g.x * r.z + g.y * r.w - g.z * r.x - g.w * r.y,
          -g.x * r.y + g.y * r.x + g.z * r.w - g.w * r.z, g.x * r.x + g.y * r.y + g.z * r.z + g.w * r.w};
}
GOL_HD Q4 qmul_bwd_r(Q4 q, Q4 g) {
  return {g.x * q.w + g.y * q.z - g.z * q.y - g.w * q.x, -g.x * q.z + g.y * q.w + g.z * q.x - g.w * q.y,
          g.x * q.y - g.y * q.x + g.z * q.w - g.w * q.z, g.x * q.x + g.y * q.y + g.z * q.z + g.w * q.w};
}

// Quaternion.batchRot (quaternion.py:252-265): v + 2 (w a x v + a x (a x v)), a = q.xyz
GOL_HD D3 qrot(Q4 q, D3 v) {
  const D3 a = {q.x, q.y, q.z};
  const D3 av = cross(a, v);
  return v + (av * q.w + cross(a, av)) * 2.0;
}
GOL_HD void qrot_bwd(Q4 q, D3 v, D3 g, Q4& gq, D3& gv) {
  const D3 a = {q.x, q.y, q.z};
  const D3 av = cross(a, v);
  const D3 g2 = g * 2.0;                       // gradient of w av + a x av
  const D3 g_av = g2 * q.w + cross(g2, a);     // a x av w.r.t. av
  const D3 g_a = cross(av, g2) + cross(v, g_av);
  gv = g + cross(g_av, a);
  gq = {g_a.x, g_a.y, g_a.z, dot(av, g2)};
}

// cosines and sines of the half angles (-0.5, 0.5, 0.5) r of Quaternion.batchFromXYZ (quaternion.py:296-298).  One sincos
// body serves the three angles (a loop that is kept a loop): the accurate double-precision sincos holds some forty
// constants in scalar registers, and one inlined copy per angle and call site is what fills the scalar register file.
struct HalfTrig {
  double c0, c1, c2, s0, s1, s2;
};
GOL_HD HalfTrig half_trig(D3 r) {
  HalfTrig t = {1.0, 1.0, 1.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int i = 0; i < 3; ++i) {
    const double h = i == 0 ? -0.5 * r.x : i == 1 ? 0.5 * r.y : 0.5 * r.z;
    double s, c;
    sincos(h, &s, &c);
    if (i == 0) { t.c0 = c; t.s0 = s; }
    else if (i == 1) { t.c1 = c; t.s1 = s; }
    else { t.c2 = c; t.s2 = s; }
  }
  return t;
}

// Quaternion.batchFromXYZ (quaternion.py:285-320)
GOL_HD Q4 from_xyz(const HalfTrig& t) {
  const double c0 = t.c0, c1 = t.c1, c2 = t.c2, s0 = t.s0, s1 = t.s1, s2 = t.s2;
  return {-s0 * (c1 * c2) - c0 * (s1 * s2), c0 * (s1 * c2) - s0 * (c1 * s2), c0 * (c1 * s2) + s0 * (s1 * c2),
          c0 * (c1 * c2) - s0 * (s1 * s2)};
}
// g: the gradient of the quaternion -> the gradient of the three angles r
GOL_HD D3 from_xyz_bwd(const HalfTrig& t, Q4 g) {
  const double c0 = t.c0, c1 = t.c1, c2 = t.c2, s0 = t.s0, s1 = t.s1, s2 = t.s2;
  const Q4 q = {-s0 * c1 * c2 - c0 * s1 * s2, c0 * s1 * c2 - s0 * c1 * s2, c0 * c1 * s2 + s0 * s1 * c2,
                c0 * c1 * c2 - s0 * s1 * s2};
  const double g0 = -g.x * q.w - g.y * q.z + g.z * q.y + g.w * q.x;
  const double g1 = g.x * (s0 * s1 * c2 - c0 * c1 * s2) + g.y * (c0 * c1 * c2 + s0 * s1 * s2) +
                    g.z * (s0 * c1 * c2 - c0 * s1 * s2) - g.w * (c0 * s1 * c2 + s0 * c1 * s2);
  const double g2 = g.x * (s0 * c1 * s2 - c0 * s1 * c2) - g.y * (c0 * s1 * s2 + s0 * c1 * c2) + g.z * q.w - g.w * q.z;
  return {-0.5 * g0, 0.5 * g1, 0.5 * g2};
}

// a child's state from its parent's and its local transform (lbs.py:366-377)
GOL_HD State compose(const State& p, D3 lt, Q4 lr, double ls) { return {qrot(p.q, lt * p.s) + p.t, qmul(p.q, lr), p.s * ls}; }
// g: the gradient of the child's state.  gp: what it adds to the parent's; glt, glr, gls: the local transform's
GOL_HD void compose_bwd(const State& p, D3 lt, Q4 lr, double ls, const State& g, State& gp, D3& glt, Q4& glr, double& gls) {
  Q4 gq;
  D3 gu;
  qrot_bwd(p.q, lt * p.s, g.t, gq, gu);
  gp.t = g.t;
  gp.q = gq + qmul_bwd_q(lr, g.q);
  gp.s = dot(gu, lt) + g.s * ls;
  glt = gu * p.s;
  glr = qmul_bwd_r(p.q, g.q);
  gls = g.s * p.s;
}

// states_to_matrix (lbs.py:388-429) with the bind inverse (bt, br, bs of :392-394) given: m[3][4] row-major
GOL_HD void state_to_matrix(const State& s, const State& binv, double m[12]) {
  const Q4 r = qmul(s.q, binv.q);
  const double ts = s.s * binv.s;
  const D3 tt = qrot(s.q, binv.t * s.s) + s.t;
  const double twx = 2.0 * r.x * r.w, twy = 2.0 * r.y * r.w, twz = 2.0 * r.z * r.w, txx = 2.0 * r.x * r.x,
               txy = 2.0 * r.y * r.x, txz = 2.0 * r.z * r.x, tyy = 2.0 * r.y * r.y, tyz = 2.0 * r.z * r.y,
               tzz = 2.0 * r.z * r.z;
  m[0] = (1.0 - (tyy + tzz)) * ts; m[1] = (txy - twz) * ts; m[2] = (txz + twy) * ts; m[3] = tt.x;
  m[4] = (txy + twz) * ts; m[5] = (1.0 - (txx + tzz)) * ts; m[6] = (tyz - twx) * ts; m[7] = tt.y;
  m[8] = (txz - twy) * ts; m[9] = (tyz + twx) * ts; m[10] = (1.0 - (txx + tyy)) * ts; m[11] = tt.z;
}
// gm[12] -> the gradient of the state (returned, not accumulated)
GOL_HD State state_to_matrix_bwd(const State& s, const State& binv, const double gm[12]) {
  const Q4 r = qmul(s.q, binv.q);
  const double ts = s.s * binv.s;
  const double x = r.x, y = r.y, z = r.z, w = r.w;
  const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
                       2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                       2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)};
  double g[9], g_ts = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      g_ts += gm[4 * i + j] * R[3 * i + j];
      g[3 * i + j] = gm[4 * i + j] * ts;
    }
  const Q4 gr = {2.0 * (y * (g[1] + g[3]) + z * (g[2] + g[6]) - 2.0 * x * (g[4] + g[8]) + w * (g[7] - g[5])),
                 2.0 * (x * (g[1] + g[3]) + z * (g[5] + g[7]) - 2.0 * y * (g[0] + g[8]) + w * (g[2] - g[6])),
                 2.0 * (x * (g[2] + g[6]) + y * (g[5] + g[7]) - 2.0 * z * (g[0] + g[4]) + w * (g[3] - g[1])),
                 2.0 * (x * (g[7] - g[5]) + y * (g[2] - g[6]) + z * (g[3] - g[1]))};
  const D3 gtt = {gm[3], gm[7], gm[11]};
  Q4 gq;
  D3 gu;
  qrot_bwd(s.q, binv.t * s.s, gtt, gq, gu);
  return {gtt, gq + qmul_bwd_q(binv.q, gr), g_ts * binv.s + dot(gu, binv.t)};
}

// the local transform of a joint from its 7 parameters (lbs.py:353-361)
GOL_HD void local_transform(const double p[7], D3 offset, Q4 pre, D3& lt, Q4& lr, double& ls) {
  lt = D3{p[0], p[1], p[2]} + offset;
  lr = qmul(pre, from_xyz(half_trig({p[3], p[4], p[5]})));
  ls = exp2(p[6]);
}
// ls: the forward's 2^p[6]
GOL_HD void local_transform_bwd(const double p[7], Q4 pre, double ls, D3 glt, Q4 glr, double gls, double gp[7]) {
  const D3 gr = from_xyz_bwd(half_trig({p[3], p[4], p[5]}), qmul_bwd_r(pre, glr));
  gp[0] = glt.x; gp[1] = glt.y; gp[2] = glt.z;
  gp[3] = gr.x; gp[4] = gr.y; gp[5] = gr.z;
  gp[6] = gls * ls * 0.6931471805599453094;
}

}  // namespace gol_lbs
