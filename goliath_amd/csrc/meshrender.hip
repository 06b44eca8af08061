// meshrender.hip -- textured mesh render on top of gol_mesh_raster's images: forward, interior backward and the
// edge-gradient term, gfx950 (wave64).
//
// Replaces the host-side PyTorch composition of goliath_amd.meshraster.RenderLayer (the drtk layer of the reference,
// ca_code/utils/render_drtk.py:44-70): interpolate(vt, vti) -> grid_sample(tex) * mask, the differentiable re-evaluation
// of depth / barycentrics (meshraster.render) and the edge-gradient estimator (meshraster._EdgeGrad), with the same
// arithmetic and the same discrete decisions.  Three kernels, all one thread per pixel:
//   fwd   vt_img = sum_k bary_k (2 vt[vti[f,k]] - 1); render = bilinear(tex, vt_img) * mask (grid_sample, bilinear,
//         align_corners=False, zero padding); mask = (index >= 0).  Linear pixel order, grid-stride.
//   bwd   one 256-thread workgroup per 16x16 tile, each wave an 8x8 block (a compact block touches few faces).  g_tex:
//         four bilinear taps per pixel and channel, float atomics straight into the planar [B,C,Ht,Wt] gradient.
//         g_v_pix: the uv gradient -> barycentrics -> the perspective-correct function of the face's nine coordinates;
//         the lanes of a wave that share a face sum their nine values across the wave (DPP) before three atomic
//         instructions (four lanes each), one loop step per distinct face of the wave.
//   edge  the right and lower neighbour pairs whose face indices differ, compacted per wave by ballot into LDS; each
//         lane then resolves one pair (occluder, crossing edge, weight, coefficient) and adds coef * d x* / d (edge
//         endpoints, image coordinates) with four atomics.
// Float-atomic arrival order makes g_tex and g_v_pix nondeterministic in the last bits from run to run.
#include "gol_common.h"

namespace {

constexpr int kMaxGrid = 8192;   // grid-stride cap of the linear-order kernels

inline int gol_grid(size_t n) { return (int)((n + 255) / 256 < (size_t)kMaxGrid ? (n + 255) / 256 : (size_t)kMaxGrid); }

struct Taps {
  int x0, y0;            // north-west tap
  float ix, iy;          // unnormalised sample position
  float wx0, wx1, wy0, wy1;
};

// grid_sample's unnormalisation (align_corners=False): x = ((u + 1) W - 1) / 2.  Positions more than one texel outside
// the texture are clamped to a point where both taps of the axis are outside as well: the sample and its gradient are 0
// either way, and the integer conversion stays in range.
__device__ __forceinline__ Taps gol_taps(float u, float v, int Ht, int Wt) {
  Taps t;
  t.ix = fminf(fmaxf(((u + 1.f) * (float)Wt - 1.f) * 0.5f, -2.f), (float)Wt + 1.f);
  t.iy = fminf(fmaxf(((v + 1.f) * (float)Ht - 1.f) * 0.5f, -2.f), (float)Ht + 1.f);
  t.x0 = (int)floorf(t.ix);
  t.y0 = (int)floorf(t.iy);
  t.wx1 = t.ix - (float)t.x0; t.wx0 = (float)(t.x0 + 1) - t.ix;
  t.wy1 = t.iy - (float)t.y0; t.wy0 = (float)(t.y0 + 1) - t.iy;
  return t;
}

// the four tap values of one plane (0 outside)
__device__ __forceinline__ void gol_tap_values(const float* __restrict__ plane, const Taps& t, int Ht, int Wt, float& v00,
                                               float& v01, float& v10, float& v11) {
  const bool x0in = t.x0 >= 0 && t.x0 < Wt, x1in = t.x0 + 1 >= 0 && t.x0 + 1 < Wt;
  const bool y0in = t.y0 >= 0 && t.y0 < Ht, y1in = t.y0 + 1 >= 0 && t.y0 + 1 < Ht;
  const size_t r0 = (size_t)t.y0 * Wt, r1 = r0 + Wt;
  v00 = (x0in && y0in) ? plane[r0 + t.x0] : 0.f;
  v01 = (x1in && y0in) ? plane[r0 + t.x0 + 1] : 0.f;
  v10 = (x0in && y1in) ? plane[r1 + t.x0] : 0.f;
  v11 = (x1in && y1in) ? plane[r1 + t.x0 + 1] : 0.f;
}

// face f's vertex ids (vi) and uv ids (vti), validated: false = treat the pixel as empty
__device__ __forceinline__ bool gol_face_ids(int f, int F, int N, const int32_t* __restrict__ ids, int& i0, int& i1, int& i2) {
  if (f < 0 || f >= F) return false;
  i0 = ids[3 * f]; i1 = ids[3 * f + 1]; i2 = ids[3 * f + 2];
  return i0 >= 0 && i0 < N && i1 >= 0 && i1 < N && i2 >= 0 && i2 < N;
}

__global__ __launch_bounds__(256) void mesh_render_fwd_kernel(int B, int F, int Vt, int C, int H, int W, int Ht, int Wt,
                                                              const float* __restrict__ vt,
                                                              const int32_t* __restrict__ vti,
                                                              const float* __restrict__ tex,
                                                              const int32_t* __restrict__ index_img,
                                                              const float* __restrict__ bary_img,
                                                              float* __restrict__ vt_img, float* __restrict__ render,
                                                              float* __restrict__ mask) {
  const size_t hw = (size_t)H * W, n = (size_t)B * hw, thw = (size_t)Ht * Wt;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
    const size_t b = p / hw, pix = p - b * hw;
    int t0, t1, t2;
    const bool hit = gol_face_ids(index_img[p], F, Vt, vti, t0, t1, t2);
    float u = 0.f, v = 0.f;
    if (hit) {
      const float* bp = bary_img + b * 3 * hw + pix;
      const float b0 = bp[0], b1 = bp[hw], b2 = bp[2 * hw];
      u = (2.f * vt[2 * t0] - 1.f) * b0 + (2.f * vt[2 * t1] - 1.f) * b1 + (2.f * vt[2 * t2] - 1.f) * b2;
      v = (2.f * vt[2 * t0 + 1] - 1.f) * b0 + (2.f * vt[2 * t1 + 1] - 1.f) * b1 + (2.f * vt[2 * t2 + 1] - 1.f) * b2;
    }
    vt_img[b * 2 * hw + pix] = u;
    vt_img[(b * 2 + 1) * hw + pix] = v;
    mask[p] = hit ? 1.f : 0.f;
    float* out = render + b * C * hw + pix;
    if (hit) {
      const Taps t = gol_taps(u, v, Ht, Wt);
      const float* plane = tex + b * C * thw;
      for (int c = 0; c < C; ++c, plane += thw) {
        float v00, v01, v10, v11;
        gol_tap_values(plane, t, Ht, Wt, v00, v01, v10, v11);
        out[c * hw] = v00 * (t.wx0 * t.wy0) + v01 * (t.wx1 * t.wy0) + v10 * (t.wx0 * t.wy1) + v11 * (t.wx1 * t.wy1);
      }
    } else {
      for (int c = 0; c < C; ++c) out[c * hw] = 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void mesh_render_bwd_kernel(
    int V, int F, int Vt, int C, int H, int W, int Ht, int Wt, int tiles_x, const float* __restrict__ v_pix,
    const int32_t* __restrict__ vi, const float* __restrict__ vt, const int32_t* __restrict__ vti,
    const float* __restrict__ tex, const int32_t* __restrict__ index_img, const float* __restrict__ bary_img,
    const float* __restrict__ g_render, const float* __restrict__ g_vt_img, const float* __restrict__ g_bary_img,
    const float* __restrict__ g_depth_img, float* __restrict__ g_tex, float* __restrict__ g_v_pix) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int j = tx * 16 + (wv & 1) * 8 + (lane & 7), i = ty * 16 + (wv >> 1) * 8 + (lane >> 3);
  const size_t hw = (size_t)H * W, thw = (size_t)Ht * Wt, pix = (size_t)i * W + j, p = (size_t)b * hw + pix;
  int f = -1, ia = 0, ib = 0, ic = 0, t0 = 0, t1 = 0, t2 = 0;
  bool hit = false;
  if (i < H && j < W) {
    f = index_img[p];
    hit = gol_face_ids(f, F, V, vi, ia, ib, ic) && gol_face_ids(f, F, Vt, vti, t0, t1, t2);
  }
  if (gol_ballot(hit) == 0ull) return;   // wave-uniform: nothing of this 8x8 block is covered
  float g[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // (ax, ay, az, bx, by, bz, cx, cy, cz)
  if (hit) {
    // uv of the forward (from the rasterizer's barycentrics) and the texture taps
    const float* bp = bary_img + (size_t)b * 3 * hw + pix;
    const float r0 = bp[0], r1 = bp[hw], r2 = bp[2 * hw];
    const float u0 = 2.f * vt[2 * t0] - 1.f, u1 = 2.f * vt[2 * t1] - 1.f, u2 = 2.f * vt[2 * t2] - 1.f;
    const float w0 = 2.f * vt[2 * t0 + 1] - 1.f, w1 = 2.f * vt[2 * t1 + 1] - 1.f, w2 = 2.f * vt[2 * t2 + 1] - 1.f;
    const float u = u0 * r0 + u1 * r1 + u2 * r2, v = w0 * r0 + w1 * r1 + w2 * r2;
    float gu = 0.f, gv = 0.f;
    if (g_render) {
      const Taps t = gol_taps(u, v, Ht, Wt);
      const bool x0in = t.x0 >= 0 && t.x0 < Wt, x1in = t.x0 + 1 >= 0 && t.x0 + 1 < Wt;
      const bool y0in = t.y0 >= 0 && t.y0 < Ht, y1in = t.y0 + 1 >= 0 && t.y0 + 1 < Ht;
      const size_t o00 = (size_t)t.y0 * Wt + t.x0, o10 = o00 + Wt;
      const float* plane = tex + (size_t)b * C * thw;
      float* gplane = g_tex ? g_tex + (size_t)b * C * thw : nullptr;
      const float* gr = g_render + (size_t)b * C * hw + pix;
      float gix = 0.f, giy = 0.f;
      for (int c = 0; c < C; ++c, plane += thw) {
        const float go = gr[c * hw];
        if (go == 0.f) continue;
        float v00, v01, v10, v11;
        gol_tap_values(plane, t, Ht, Wt, v00, v01, v10, v11);
        gix += go * ((v01 - v00) * t.wy0 + (v11 - v10) * t.wy1);
        giy += go * ((v10 - v00) * t.wx0 + (v11 - v01) * t.wx1);
        if (gplane) {
          float* gp = gplane + c * thw;
          if (x0in && y0in) atomicAdd(gp + o00, go * (t.wx0 * t.wy0));
          if (x1in && y0in) atomicAdd(gp + o00 + 1, go * (t.wx1 * t.wy0));
          if (x0in && y1in) atomicAdd(gp + o10, go * (t.wx0 * t.wy1));
          if (x1in && y1in) atomicAdd(gp + o10 + 1, go * (t.wx1 * t.wy1));
        }
      }
      gu = gix * (0.5f * (float)Wt);
      gv = giy * (0.5f * (float)Ht);
    }
    if (g_vt_img) {
      gu += g_vt_img[(size_t)b * 2 * hw + pix];
      gv += g_vt_img[((size_t)b * 2 + 1) * hw + pix];
    }
    if (g_v_pix) {
      float gb0 = gu * u0 + gv * w0, gb1 = gu * u1 + gv * w1, gb2 = gu * u2 + gv * w2;
      if (g_bary_img) {
        const float* gbp = g_bary_img + (size_t)b * 3 * hw + pix;
        gb0 += gbp[0]; gb1 += gbp[hw]; gb2 += gbp[2 * hw];
      }
      const float gd = g_depth_img ? g_depth_img[p] : 0.f;
      // meshraster.render: barycentrics anchored at a, sampled at the pixel centre, perspective-correct
      const float* P = v_pix + (size_t)b * V * 3;
      const float ax = P[3 * ia], ay = P[3 * ia + 1], az = P[3 * ia + 2];
      const float bx = P[3 * ib], by = P[3 * ib + 1], bz = P[3 * ib + 2];
      const float cx = P[3 * ic], cy = P[3 * ic + 1], cz = P[3 * ic + 2];
      const float area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
      const float dx = ((float)j + 0.5f) - ax, dy = ((float)i + 0.5f) - ay;
      const float b1 = ((cy - ay) * dx + (ax - cx) * dy) / area;
      const float b2 = ((ay - by) * dx + (bx - ax) * dy) / area;
      const float b0 = 1.f - b1 - b2;
      const float q0 = b0 / az, q1 = b1 / bz, q2 = b2 / cz;
      const float iz = q0 + q1 + q2;
      // bary_k = q_k / iz, depth = 1 / iz  ->  d/dq_k = (gb_k - sum_j gb_j bary_j - gd depth) / iz
      const float s = (gb0 * q0 + gb1 * q1 + gb2 * q2) / iz + gd / iz;
      const float gq0 = (gb0 - s) / iz, gq1 = (gb1 - s) / iz, gq2 = (gb2 - s) / iz;
      g[2] = -gq0 * q0 / az; g[5] = -gq1 * q1 / bz; g[8] = -gq2 * q2 / cz;
      const float G1 = gq1 / bz - gq0 / az, G2 = gq2 / cz - gq0 / az;   // b0 = 1 - b1 - b2
      const float gN1 = G1 / area, gN2 = G2 / area, gA = -(G1 * b1 + G2 * b2) / area;
      g[0] = gN1 * (dy - (cy - ay)) - gN2 * ((ay - by) + dy) + gA * (by - cy);
      g[1] = -gN1 * (dx + (ax - cx)) + gN2 * (dx - (bx - ax)) + gA * (cx - bx);
      g[3] = gN2 * dy + gA * (cy - ay);
      g[4] = -gN2 * dx + gA * (ax - cx);
      g[6] = -gN1 * dy + gA * (ay - by);
      g[7] = gN1 * dx + gA * (bx - ax);
    }
  }
  if (!g_v_pix) return;
  // per distinct face of the wave: a full-wave sum of the lanes on that face, then 9 atomics from lanes 15/31/47/63
  float* G = g_v_pix + (size_t)b * V * 3;
  unsigned long long todo = gol_ballot(hit);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int f0 = __builtin_amdgcn_readlane(f, leader);
    const bool mine = hit && f == f0;
    const unsigned long long m = gol_ballot(mine);
    todo &= ~m;
    if (__popcll(m) == 1) {
      if (mine) {
        const int id[3] = {ia, ib, ic};
#pragma unroll
        for (int k = 0; k < 9; ++k) atomicAdd(G + 3 * id[k / 3] + k % 3, g[k]);
      }
      continue;
    }
    const int va = __builtin_amdgcn_readlane(ia, leader), vb = __builtin_amdgcn_readlane(ib, leader),
              vc = __builtin_amdgcn_readlane(ic, leader);
    float e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = mine ? g[k] : 0.f;
    const float s0 = gol_wave_sum4(e[0], e[1], e[2], e[3]);   // lanes 15, 31, 47, 63 = ax, ay, az, bx
    const float s1 = gol_wave_sum4(e[4], e[5], e[6], e[7]);   // by, bz, cx, cy
    const float s2 = gol_wave_sum_to_lane63(e[8]);            // cz
    const int row = lane >> 4;
    if ((lane & 15) == 15) {
      // component k = 4 * step + row of (ax, ay, az, bx, by, bz, cx, cy, cz)
      const int k0 = row, k1 = 4 + row;
      atomicAdd(G + 3 * (k0 < 3 ? va : vb) + (k0 < 3 ? k0 : 0), s0);
      atomicAdd(G + 3 * (k1 < 6 ? vb : vc) + (k1 < 6 ? k1 - 3 : k1 - 6), s1);
      if (lane == 63) atomicAdd(G + 3 * vc + 2, s2);
    }
  }
}

__global__ __launch_bounds__(256) void mesh_render_edge_kernel(int B, int V, int F, int C, int H, int W,
                                                               const float* __restrict__ v_pix,
                                                               const int32_t* __restrict__ vi,
                                                               const int32_t* __restrict__ index_img,
                                                               const float* __restrict__ depth_img,
                                                               const float* __restrict__ render,
                                                               const float* __restrict__ g_render,
                                                               float* __restrict__ g_v_pix, int32_t* __restrict__ stats) {
  __shared__ int32_t s_slot[4][128];   // per wave: compacted (source lane | axis << 6)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const size_t hw = (size_t)H * W, n = (size_t)B * hw;
  for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {   // block-uniform
    const size_t p = base + threadIdx.x;
    bool cr = false, cd = false;
    if (p < n) {
      const size_t pix = p % hw;
      const int i = (int)(pix / W), j = (int)(pix - (size_t)i * W);
      const int ip = index_img[p];
      cr = j + 1 < W && index_img[p + 1] != ip;
      cd = i + 1 < H && index_img[p + W] != ip;
    }
    const unsigned long long m0 = gol_ballot(cr), m1 = gol_ballot(cd);
    const int n0 = __popcll(m0), ncand = n0 + __popcll(m1);
    if (cr) s_slot[wv][__popcll(m0 & lt)] = lane;
    if (cd) s_slot[wv][n0 + __popcll(m1 & lt)] = lane | 64;
    __syncthreads();
    int n_edges = 0, n_dropped = 0;
    for (int k = lane; k < ncand; k += 64) {
      const int slot = s_slot[wv][k], axis = slot >> 6;
      const size_t pp = base + (size_t)wv * 64 + (slot & 63);
      const size_t b = pp / hw, pix = pp - b * hw;
      const int i = (int)(pix / W), j = (int)(pix - (size_t)i * W);
      const size_t pq = axis == 0 ? pp + 1 : pp + W;
      int fp = index_img[pp], fq = index_img[pq];
      int tp[3], tq[3];
      const bool hp = gol_face_ids(fp, F, V, vi, tp[0], tp[1], tp[2]);
      const bool hq = gol_face_ids(fq, F, V, vi, tq[0], tq[1], tq[2]);
      int shared = 0;
      if (hp && hq)
#pragma unroll
        for (int a = 0; a < 3; ++a) shared += (tp[a] == tq[0] || tp[a] == tq[1] || tp[a] == tq[2]) ? 1 : 0;
      if ((hp && hq && shared >= 2) || (!hp && !hq)) continue;   // a shared mesh edge: no discontinuity
      ++n_edges;
      const float zp = hp ? depth_img[pp] : INFINITY, zq = hq ? depth_img[pq] : INFINITY;
      const int* tri = zp <= zq ? tp : tq;                       // the occluder (an empty pixel never occludes)
      const float* P = v_pix + b * (size_t)V * 3;
      const int al = axis, ac = 1 - axis;                        // along the segment p -> q / across it
      const float c_fix = (float)(axis == 0 ? i : j) + 0.5f;
      const float s_mid = ((float)(axis == 0 ? j : i) + 0.5f) + 0.5f;
      float best = INFINITY, bt = 0.f, bdal = 0.f, bdac = 1.f;
      int be = 0;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const float* e0 = P + 3 * tri[e];
        const float* e1 = P + 3 * tri[(e + 1) % 3];
        const float a0 = e0[ac], a1 = e1[ac], d_ac = a1 - a0;
        if (!((a0 - c_fix) * (a1 - c_fix) <= 0.f && d_ac != 0.f)) continue;
        const float t = (c_fix - a0) / d_ac, d_al = e1[al] - e0[al];
        const float dist = fabsf(e0[al] + t * d_al - s_mid);
        if (dist < best) { best = dist; be = e; bt = t; bdal = d_al; bdac = d_ac; }   // first argmin
      }
      if (!(best <= 1.f)) { ++n_dropped; continue; }
      const float weight = bdac * bdac / fmaxf(bdac * bdac + bdal * bdal, 1e-30f);
      float coef = 0.f;
      const float* rp = render + b * (size_t)C * hw + pix;
      const float* gp = g_render + b * (size_t)C * hw + pix;
      const size_t dq = pq - pp;
      for (int c = 0; c < C; ++c)
        coef += 0.5f * (gp[c * hw] + gp[c * hw + dq]) * (rp[c * hw] - rp[c * hw + dq]);
      coef *= weight;
      // x* = e0_al + t (e1_al - e0_al), t = (c - e0_ac) / (e1_ac - e0_ac)
      float* G = g_v_pix + b * (size_t)V * 3;
      const int v0 = tri[be], v1 = tri[(be + 1) % 3];
      atomicAdd(G + 3 * v0 + al, coef * (1.f - bt));
      atomicAdd(G + 3 * v1 + al, coef * bt);
      atomicAdd(G + 3 * v0 + ac, coef * bdal * (bt - 1.f) / bdac);
      atomicAdd(G + 3 * v1 + ac, -coef * bdal * bt / bdac);
    }
    if (stats) {
      if (n_edges) atomicAdd(&stats[0], n_edges);
      if (n_dropped) atomicAdd(&stats[1], n_dropped);
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int gol_mesh_render_fwd(int B, int F, int Vt, int C, int H, int W, int Ht, int Wt, const float* vt,
                                   const int32_t* vti, const float* tex, const int32_t* index_img, const float* bary_img,
                                   float* vt_img, float* render, float* mask, void* stream) {
  GOL_REQUIRE(B >= 0 && F >= 0 && Vt >= 0 && C >= 1 && H > 0 && W > 0 && Ht > 0 && Wt > 0, "bad size");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(index_img && bary_img && tex && vt_img && render && mask, "null pointer");
  GOL_REQUIRE(F == 0 || (vt && vti), "null uv table");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)B * H * W;
  mesh_render_fwd_kernel<<<gol_grid(n), 256, 0, s>>>(
      B, F, Vt, C, H, W, Ht, Wt, vt, vti, tex, index_img, bary_img, vt_img, render, mask);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_mesh_render_bwd(int B, int V, int F, int Vt, int C, int H, int W, int Ht, int Wt, const float* v_pix,
                                   const int32_t* vi, const float* vt, const int32_t* vti, const float* tex,
                                   const int32_t* index_img, const float* bary_img, const float* g_render,
                                   const float* g_vt_img, const float* g_bary_img, const float* g_depth_img,
                                   float* g_tex, float* g_v_pix, void* stream) {
  GOL_REQUIRE(B >= 0 && V >= 0 && F >= 0 && Vt >= 0 && C >= 1 && H > 0 && W > 0 && Ht > 0 && Wt > 0, "bad size");
  GOL_REQUIRE(B <= 65535, "size out of range");
  if (B == 0 || F == 0 || (!g_tex && !g_v_pix)) return GOL_OK;
  GOL_REQUIRE(index_img && bary_img && vt && vti && vi && tex, "null input");
  GOL_REQUIRE(!g_v_pix || v_pix, "g_v_pix needs v_pix");
  if (!g_render && !g_vt_img && !g_bary_img && !g_depth_img) return GOL_OK;
  const int tiles_x = gol_cdiv(W, 16), tiles = tiles_x * gol_cdiv(H, 16);
  mesh_render_bwd_kernel<<<dim3(tiles, B), 256, 0, (hipStream_t)stream>>>(
      V, F, Vt, C, H, W, Ht, Wt, tiles_x, v_pix, vi, vt, vti, tex, index_img, bary_img, g_render, g_vt_img, g_bary_img,
      g_depth_img, g_tex, g_v_pix);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_mesh_render_edge_bwd(int B, int V, int F, int C, int H, int W, const float* v_pix, const int32_t* vi,
                                        const int32_t* index_img, const float* depth_img, const float* render,
                                        const float* g_render, float* g_v_pix, int32_t* edge_stats, void* stream) {
  GOL_REQUIRE(B >= 0 && V >= 0 && F >= 0 && C >= 1 && H > 0 && W > 0, "bad size");
  if (B == 0 || F == 0) return GOL_OK;
  GOL_REQUIRE(v_pix && vi && index_img && depth_img && render && g_render && g_v_pix, "null pointer");
  const size_t n = (size_t)B * H * W;
  mesh_render_edge_kernel<<<gol_grid(n), 256, 0, (hipStream_t)stream>>>(
      B, V, F, C, H, W, v_pix, vi, index_img, depth_img, render, g_render, g_v_pix, edge_stats);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
