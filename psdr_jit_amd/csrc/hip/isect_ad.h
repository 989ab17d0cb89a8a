// isect_ad.h — Scene.unit_ray_intersectAD for a batch of rays: the solid-angle AD form of Scene::ray_intersect
// (reference src/scene/scene.cpp:774-797, ad = true, path_space = false), its forward tangent and its hand-written adjoint.
//
// The record is the 24-float layout of PSDR_ITS_STRIDE.  Unlike the C record (barycentrics of the tracer, t = |p - o|) its
// (u, v, t) come from re-intersecting the hit triangle (ray_intersect_triangle<true>, reference include/psdr/utils.h:83-93),
// so t, p, the shading frame, wi and uv move with the triangle's rows and with the ray.  The texture coordinates of the
// triangle's corners are constants (the reference gathers them from a detached array).
//
// isect_ad_eval is the forward in either number type (Dual: one tangent, render_kernels.h::k_intersect_ad); isect_ad_adjoint is its
// transpose, stage by stage, in float registers from the same rows (render_kernels.h::k_intersect_adj).  tests/test_gpu_intersect_ad.py
// checks the two against each other (<J^T w, v> = <w, J v>) and against a float64 torch restatement.
#pragma once
#include "shade.h"

namespace psdr {

constexpr int kIsectRowComps = 21;      // p0 e1 e2 n0 n1 n2 face_normal of a 22-float triangle row; face_area gets nothing (J = 1)

template <typename R> struct IsectGeom { Vec3<R> p0, e1, e2, n0, n1, n2, fn; };
// constant part of a hit's rows: corner texture coordinates (uv0, uv1, uv2), the flat-shading bit, mesh and original triangle id
struct IsectConst { float uv[6]; bool flat; int mesh; };

template <typename R> struct IsectOut { R t; Vec3<R> p, fs, ft, fn, wi; R tu, tv; };

// the shading-row part of a slot (make_its reads the same words; that function stays as it is - its code generation is tuned)
template <bool AD, int LDS> PSDR_DEV void isect_load(const SceneView<LDS> &S, int slot, IsectGeom<Num<AD>> &g, IsectConst &c) {
    const SceneTables &T = *S.T;
    load_geom<AD, LDS>(S, slot, g.p0, g.e1, g.e2);
    const int w = T.shade_off + 6 * slot;
    const float4 s0 = S.ld(w), s1 = S.ld(w + 1), s2 = S.ld(w + 2), s3 = S.ld(w + 3), s4 = S.ld(w + 4), s5 = S.ld(w + 5);
    const Vec3f n0(s0.x, s0.y, s0.z), n1(s1.x, s1.y, s1.z), n2(s2.x, s2.y, s2.z), fn(s3.x, s3.y, s3.z);
    if constexpr (AD) {
        if (S.tan_on()) {
            const float4 tc = S.tanw(slot, 2), td = S.tanw(slot, 3), te = S.tanw(slot, 4), tf = S.tanw(slot, 5);
            g.n0 = make_dual(n0, Vec3f(tc.y, tc.z, tc.w)); g.n1 = make_dual(n1, Vec3f(td.x, td.y, td.z));
            g.n2 = make_dual(n2, Vec3f(td.w, te.x, te.y)); g.fn = make_dual(fn, Vec3f(te.z, te.w, tf.x));
        } else { g.n0 = promote(n0); g.n1 = promote(n1); g.n2 = promote(n2); g.fn = promote(fn); }
    } else { g.n0 = n0; g.n1 = n1; g.n2 = n2; g.fn = fn; }
    c.uv[0] = s4.x; c.uv[1] = s4.y; c.uv[2] = s4.z; c.uv[3] = s4.w; c.uv[4] = s5.x; c.uv[5] = s5.y;
    c.flat = (__float_as_int(s2.w) & 1) != 0;
    c.mesh = __float_as_int(s1.w);
}

// scene.cpp:774-797: (u, v, t) by Moller-Trumbore, p = o + t d, the normalised blend of the vertex normals (the face normal on flat
// meshes), the frame from dp_du when the uv parameterisation is non-degenerate (Duff's coordinate_system otherwise), wi = to_local(-d),
// uv = the blend of the corner texture coordinates with the differentiable (u, v)
template <typename R>
PSDR_DEV void isect_ad_eval(const Vec3<R> &o, const Vec3<R> &d, const IsectGeom<R> &g, const IsectConst &c, IsectOut<R> &out) {
    R u, v, t;
    ray_tri_uvt<R>(g.p0, g.e1, g.e2, o, d, u, v, t);
    out.t = t;
    out.p = Vec3<R>(fma_(d.x, t, o.x), fma_(d.y, t, o.y), fma_(d.z, t, o.z));
    const Vec3<R> sh_n = c.flat ? g.fn : normalize(madd3(g.n1 - g.n0, u, g.n2 - g.n0, v, g.n0));
    const float du0x = c.uv[2] - c.uv[0], du0y = c.uv[3] - c.uv[1], du1x = c.uv[4] - c.uv[0], du1y = c.uv[5] - c.uv[1];
    out.tu = fma_(R(du0x), u, fma_(R(du1x), v, R(c.uv[0])));
    out.tv = fma_(R(du0y), u, fma_(R(du1y), v, R(c.uv[1])));
    const float det = fma_(du0x, du1y, -(du0y * du1x));
    if (det != 0.f) {
        const float inv_det = 1.f / det;
        const Vec3<R> dp_du = (g.e1 * R(du1y) - g.e2 * R(du0y)) * R(inv_det);
        out.fs = normalize(dp_du - sh_n * dot(sh_n, dp_du));
        out.ft = cross(sh_n, out.fs);
    } else {
        coordinate_system(sh_n, out.fs, out.ft);
    }
    out.fn = sh_n;
    const Vec3<R> nd = -d;
    out.wi = Vec3<R>(dot(nd, out.fs), dot(nd, out.ft), dot(nd, sh_n));
}

// The transpose of isect_ad_eval at one hit: gr = the adjoint of the 24-float record (t at 2, p 4-6, n 7-9, sh_frame 10-18, wi 19-21,
// uv 22-23; the valid / mesh / J words carry none) -> the adjoints of the rows' 21 differentiable components, of o and of d.
// The forward is recomputed in registers first; every stage below undoes one line of isect_ad_eval, last line first.
PSDR_DEV void isect_ad_adjoint(const Vec3f &o, const Vec3f &d, const IsectGeom<float> &g, const IsectConst &c, const float *gr,
                               float *g_row, Vec3f &g_o, Vec3f &g_d) {
    // ---- forward
    const Vec3f h = cross(d, g.e2);
    const float a = dot(g.e1, h);
    const float f = 1.f / a;
    const Vec3f s = o - g.p0;
    const float U = dot(s, h);
    const Vec3f q = cross(s, g.e1);
    const float Vq = dot(d, q), Tq = dot(g.e2, q);
    const float u = f * U, v = f * Vq, t = f * Tq;
    const Vec3f nb = madd3(g.n1 - g.n0, u, g.n2 - g.n0, v, g.n0);
    const float inv_len = rcp_(sqrt_(dot(nb, nb)));
    const Vec3f sh_n = c.flat ? g.fn : nb * inv_len;
    const float du0x = c.uv[2] - c.uv[0], du0y = c.uv[3] - c.uv[1], du1x = c.uv[4] - c.uv[0], du1y = c.uv[5] - c.uv[1];
    const float det = fma_(du0x, du1y, -(du0y * du1x));
    Vec3f fs, ft;
    if (det != 0.f) {
        const float inv_det = 1.f / det;
        const Vec3f dp_du = (g.e1 * du1y - g.e2 * du0y) * inv_det;
        const float k = dot(sh_n, dp_du);
        const Vec3f w = dp_du - sh_n * k;
        const float inv_w = rcp_(sqrt_(dot(w, w)));
        fs = w * inv_w;
        ft = cross(sh_n, fs);
    } else {
        coordinate_system(sh_n, fs, ft);
    }

    // ---- reverse
    Vec3f g_fs(gr[10], gr[11], gr[12]), g_ft(gr[13], gr[14], gr[15]), g_sh(gr[16], gr[17], gr[18]), g_fn(gr[7], gr[8], gr[9]);
    const Vec3f g_p(gr[4], gr[5], gr[6]), g_wi(gr[19], gr[20], gr[21]);
    float g_t = gr[2];
    // uv = uv0 + du0 u + du1 v
    float g_u = fma_(du0x, gr[22], du0y * gr[23]), g_v = fma_(du1x, gr[22], du1y * gr[23]);
    // wi = (-d.fs, -d.ft, -d.sh_n)
    const Vec3f nd = -d;
    g_fs = g_fs + nd * g_wi.x; g_ft = g_ft + nd * g_wi.y; g_sh = g_sh + nd * g_wi.z;
    g_d = -(fs * g_wi.x + ft * g_wi.y + sh_n * g_wi.z);
    Vec3f g_e1(0.f), g_e2(0.f);
    if (det != 0.f) {
        const float inv_det = 1.f / det;
        const Vec3f dp_du = (g.e1 * du1y - g.e2 * du0y) * inv_det;
        const float k = dot(sh_n, dp_du);
        const Vec3f w = dp_du - sh_n * k;
        const float inv_w = rcp_(sqrt_(dot(w, w)));
        // ft = sh_n x fs
        g_sh = g_sh + cross(fs, g_ft); g_fs = g_fs + cross(g_ft, sh_n);
        // fs = w / |w|
        const Vec3f g_w = (g_fs - fs * dot(fs, g_fs)) * inv_w;
        // w = dp_du - sh_n (sh_n . dp_du)
        const float g_k = -dot(sh_n, g_w);
        const Vec3f g_dp = g_w + sh_n * g_k;
        g_sh = g_sh - g_w * k + dp_du * g_k;
        // dp_du = (e1 du1y - e2 du0y) / det
        g_e1 = g_dp * (du1y * inv_det); g_e2 = g_dp * (-du0y * inv_det);
    } else {
        // Duff et al.: sg = sign(n.z) (detached), a = -1 / (sg + n.z), b = n.x n.y a;
        // s = (sg n.x^2 a + 1, sg b, -sg n.x), t = (b, sg + n.y^2 a, -n.y); da/dn.z = a^2
        const float nx = sh_n.x, ny = sh_n.y, nz = sh_n.z;
        const float sg = signbit_(nz) ? -1.f : 1.f;
        const float ca = -rcp_(sg + nz);
        const float g_b = fma_(sg, g_fs.y, g_ft.x);
        const float g_a = fma_(sg * nx * nx, g_fs.x, ny * ny * g_ft.y) + g_b * nx * ny;
        g_sh.x = g_sh.x + (2.f * sg * nx * ca * g_fs.x - sg * g_fs.z + g_b * ny * ca);
        g_sh.y = g_sh.y + (2.f * ny * ca * g_ft.y - g_ft.z + g_b * nx * ca);
        g_sh.z = g_sh.z + g_a * ca * ca;
    }
    // sh_n = normalize(n0 + (n1 - n0) u + (n2 - n0) v), or the face normal
    Vec3f g_n0(0.f), g_n1(0.f), g_n2(0.f);
    if (c.flat) {
        g_fn = g_fn + g_sh;
    } else {
        const Vec3f g_nb = (g_sh - sh_n * dot(sh_n, g_sh)) * inv_len;
        g_n0 = g_nb * (1.f - u - v); g_n1 = g_nb * u; g_n2 = g_nb * v;
        g_u = g_u + dot(g_nb, g.n1 - g.n0); g_v = g_v + dot(g_nb, g.n2 - g.n0);
    }
    // p = o + t d
    g_o = g_p;
    g_d = g_d + g_p * t;
    g_t = g_t + dot(g_p, d);
    // Moller-Trumbore: u = U / a, v = V / a, t = T / a; a = e1.h, h = d x e2, U = s.h, s = o - p0, q = s x e1, V = d.q, T = e2.q
    const float g_f = fma_(g_u, U, fma_(g_v, Vq, g_t * Tq));
    const float gU = g_u * f, gV = g_v * f, gT = g_t * f;
    const float g_a = -g_f * f * f;
    const Vec3f g_h = g.e1 * g_a + s * gU;
    g_e1 = g_e1 + h * g_a;
    Vec3f g_s = h * gU;
    g_d = g_d + q * gV;
    const Vec3f g_q = d * gV + g.e2 * gT;
    g_e2 = g_e2 + q * gT;
    g_s = g_s + cross(g.e1, g_q); g_e1 = g_e1 + cross(g_q, s);
    g_d = g_d + cross(g.e2, g_h); g_e2 = g_e2 + cross(g_h, d);
    g_o = g_o + g_s;
    const Vec3f g_p0 = -g_s;
    const Vec3f out[7] = {g_p0, g_e1, g_e2, g_n0, g_n1, g_n2, g_fn};
#pragma unroll
    for (int k = 0; k < 7; ++k) { g_row[3 * k] = out[k].x; g_row[3 * k + 1] = out[k].y; g_row[3 * k + 2] = out[k].z; }
}

} // namespace psdr
