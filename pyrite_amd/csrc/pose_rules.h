// pose_rules.h -- the rules of a live scene's deformation pipeline, morph -> skin -> pose -> smooth -> lamps (DESIGN.md sections
// 9g, 9h, 9p, 9q, 9r and 9s), stated once. Two layers: the arithmetic on one vector (pose_point, pose_normal_frame, blend_joints,
// blend_dual_quaternions, morph_normal_frame, signed_face_vector, ...) and, below it, what one lane of a kernel does with it over
// registers and plain pointers ("one lane's walk": pose_vertex, skin_vertex, skin_vertex_dual, add_delta, morphed_normal, add_face,
// finish_corner, pose_sphere, bounds_flag) -- which rule comes first, what an identity copies, which Flag bit a failure raises. The kernels
// (kernels/pose.hip) keep the lane mapping, the loads and stores and the bounds checks on tables in memory, and call only the
// second layer; the host rehearsals (tests/probes/deform_check.cpp, dq_skin_check.cpp) call the same functions under ASan and UBSan, so what the two
// compute can differ only in the square root and the reciprocal -- sqrt32 / rcp32 of exact_math.h on the device, std::sqrt and
// 1.0f / x on the host, bit-identical in the ranges exact_math.h names.
//
// The rule is the reference's Shape::scale and Shape::transform (shapes/mod.rs:290-344) with Normal::transform (shapes/mod.rs:
// 572-583), in f32 and in the operation order of compiler.py's _transform_point, _transform_vector, _quat_rotate, _normalize and
// _quat_from_cols. Units that include this header are built with -ffp-contract=off. A pose's last row is 0,0,0,1 (pyr_scene_pose
// refuses any other), so transform_point's division by w is a division by exactly 1 and is left out. It is compiled for the
// device and by a plain C++ compiler: no vector type and no standard container in here.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "exact_math.h"
#define PYR_POSE_HD __host__ __device__ __forceinline__
#else
#define PYR_POSE_HD inline
#endif
// a row of a device table that starts on a 16-byte boundary (the host rehearsal's tables are plain vectors: no promise there)
#if defined(__HIP_DEVICE_COMPILE__)
#define PYR_POSE_ROW16(p) ((const float*)__builtin_assume_aligned((p), 16))
#else
#define PYR_POSE_ROW16(p) (p)
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
#include <cmath>
#endif

namespace pyr {
namespace pose {

// One object's pose as the kernels read it: the matrix column-major like PyrCamera::cam_to_world, the uniform scale that comes
// first, and whether the pose is exactly the identity with scale 1 (such an object is copied from rest bit for bit:
// Normal::transform by the identity is not the identity on bits).
struct Pose {
    float m[16];
    float scale;
    uint32_t identity;
};

// The bits of the one flag word the kernels raise and pyr_scene_pose / _skin / _morph read back; the lowest bit set decides the
// refusal (live_scene.cpp scene_pose).
enum Flag : uint32_t {
    kBeyondRange = 1u,   // a bound of a moved primitive fails the coordinate check, or a table names what lies outside it
    kMorphedNormal = 2u, // a morphed normal or the tangent rebuilt against it cannot be normalised
    kSmoothedNormal = 4u, // a recomputed normal or the tangent rebuilt against it cannot be
    kBlendedRotation = 8u // a vertex's blended dual quaternion cannot be normalised (its joints' rotations cancel)
};

PYR_POSE_HD float root(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return sqrt32(x);
#else
    return std::sqrt(x);
#endif
}
PYR_POSE_HD float reciprocal(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return rcp32(x);
#else
    return 1.0f / x;
#endif
}
PYR_POSE_HD float magnitude(float x) { return x < 0.0f ? -x : x; } // fabs for everything the check below looks at (NaN stays NaN)

// creation's coordinate check on one bound (pyrite_gpu.h "Coordinates")
PYR_POSE_HD bool beyond_range(float x) { return !(magnitude(x) <= 1.0e15f); }

// cgmath normalize: v * (1 / |v|) with |v| = sqrt((x*x + y*y) + z*z)
PYR_POSE_HD void normalize(float* v) {
    const float mag = root((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const float k = reciprocal(mag);
    v[0] = v[0] * k, v[1] = v[1] * k, v[2] = v[2] * k;
}
PYR_POSE_HD float dot4(const float* a, const float* b) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }
PYR_POSE_HD void cross(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
PYR_POSE_HD void transform_vector(const float* m, const float* v, float* o) {
    o[0] = m[0] * v[0] + m[4] * v[1] + m[8] * v[2];
    o[1] = m[1] * v[0] + m[5] * v[1] + m[9] * v[2];
    o[2] = m[2] * v[0] + m[6] * v[1] + m[10] * v[2];
}
PYR_POSE_HD void transform_point(const float* m, const float* p, float* o) { // (then / w, which is 1)
    o[0] = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12];
    o[1] = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13];
    o[2] = m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14];
}
// Quaternion (s, x, y, z) * Vector3
PYR_POSE_HD void quat_rotate(const float* q, const float* vec, float* o) {
    float c[3], tmp[3], d[3];
    cross(q + 1, vec, c);
    tmp[0] = c[0] + vec[0] * q[0], tmp[1] = c[1] + vec[1] * q[0], tmp[2] = c[2] + vec[2] * q[0];
    cross(q + 1, tmp, d);
    o[0] = d[0] * 2.0f + vec[0], o[1] = d[1] * 2.0f + vec[1], o[2] = d[2] * 2.0f + vec[2];
}
// Quaternion::from(Matrix3::from_cols(c0, c1, c2)), kernels.hip's quat_from_cols
PYR_POSE_HD void quat_from_cols(const float* c0, const float* c1, const float* c2, float* q) {
    const float m00 = c0[0], m01 = c0[1], m02 = c0[2], m10 = c1[0], m11 = c1[1], m12 = c1[2], m20 = c2[0], m21 = c2[1], m22 = c2[2];
    const float trace = m00 + m11 + m22;
    if (trace >= 0.0f) {
        float s = root(1.0f + trace);
        const float w = 0.5f * s;
        s = 0.5f / s;
        q[0] = w, q[1] = (m12 - m21) * s, q[2] = (m20 - m02) * s, q[3] = (m01 - m10) * s;
    } else if (m00 > m11 && m00 > m22) {
        float s = root((m00 - m11 - m22) + 1.0f);
        const float x = 0.5f * s;
        s = 0.5f / s;
        q[0] = (m12 - m21) * s, q[1] = x, q[2] = (m10 + m01) * s, q[3] = (m02 + m20) * s;
    } else if (m11 > m22) {
        float s = root((m11 - m00 - m22) + 1.0f);
        const float y = 0.5f * s;
        s = 0.5f / s;
        q[0] = (m20 - m02) * s, q[1] = (m10 + m01) * s, q[2] = y, q[3] = (m21 + m12) * s;
    } else {
        float s = root((m22 - m00 - m11) + 1.0f);
        const float z = 0.5f * s;
        s = 0.5f / s;
        q[0] = (m01 - m10) * s, q[1] = (m02 + m20) * s, q[2] = (m21 + m12) * s, q[3] = z;
    }
}

// ---- the per-vertex arithmetic
// Shape::scale, then Shape::transform, on a vertex position
PYR_POSE_HD void pose_point(const Pose& pose, float* p) {
    const float s[3] = {p[0] * pose.scale, p[1] * pose.scale, p[2] * pose.scale};
    transform_point(pose.m, s, p);
}
// Normal::transform on a vertex normal alone (a scene that keeps no frames)
PYR_POSE_HD void pose_normal(const Pose& pose, float* n) {
    float t[3];
    transform_vector(pose.m, n, t);
    normalize(t);
    n[0] = t[0], n[1] = t[1], n[2] = t[2];
}
// Normal::transform on a vertex normal and its tangent frame
PYR_POSE_HD void pose_normal_frame(const Pose& pose, float* n, float* frame) {
    const float ex[3] = {1.0f, 0.0f, 0.0f}, ey[3] = {0.0f, 1.0f, 0.0f};
    float rx[3], ry[3], x[3], y[3];
    pose_normal(pose, n);
    quat_rotate(frame, ex, rx);
    transform_vector(pose.m, rx, x);
    normalize(x);
    quat_rotate(frame, ey, ry);
    transform_vector(pose.m, ry, y);
    normalize(y);
    quat_from_cols(x, y, n, frame);
}
// ---- the skin rule: one vertex's matrix blended from four joints, `joints` holding twelve floats a joint
// -- the upper three rows, column by column -- and j0..j3 already compared against the skin's joint count. Every entry is
// ((w0*J0 + w1*J1) + w2*J2) + w3*J3, unfused; the last row is 0,0,0,1. The vertex then takes the per-vertex rule above with
// Pose{B, 1.0f, not identity}.
PYR_POSE_HD void blend_joints(const float* joints, const uint32_t* j, const float* w, Pose& b) {
    const float *a0 = joints + 12 * (size_t)j[0], *a1 = joints + 12 * (size_t)j[1], *a2 = joints + 12 * (size_t)j[2], *a3 = joints + 12 * (size_t)j[3];
    for (int col = 0; col < 4; ++col) {
        for (int row = 0; row < 3; ++row) {
            const int e = 3 * col + row;
            b.m[4 * col + row] = ((w[0] * a0[e] + w[1] * a1[e]) + w[2] * a2[e]) + w[3] * a3[e];
        }
        b.m[4 * col + 3] = col == 3 ? 1.0f : 0.0f;
    }
    b.scale = 1.0f;
    b.identity = 0u;
}

// ---- the dual quaternion skin rule (Kavan et al. 2007): a rigid joint as a unit dual quaternion (r, d),
// eight floats -- r the rotation (s, x, y, z) of the upper 3x3, renormalised, d = 0.5 * (0, t) * r with t the translation column --
// made once per joint and frame on the host from the joint's matrix `m` (column-major, 16 floats, its upper 3x3 a rotation:
// pyr_scene_skin refuses any other for such a skin, joint_is_rotation below).
PYR_POSE_HD void joint_dual_quaternion(const float* m, float* q) {
    float r[4];
    quat_from_cols(m, m + 4, m + 8, r);
    const float k = reciprocal(root(dot4(r, r)));
    r[0] = r[0] * k, r[1] = r[1] * k, r[2] = r[2] * k, r[3] = r[3] * k;
    const float* t = m + 12;
    q[0] = r[0], q[1] = r[1], q[2] = r[2], q[3] = r[3];
    q[4] = -0.5f * ((t[0] * r[1] + t[1] * r[2]) + t[2] * r[3]);
    q[5] = 0.5f * ((t[0] * r[0] + t[1] * r[3]) - t[2] * r[2]);
    q[6] = 0.5f * ((t[1] * r[0] + t[2] * r[1]) - t[0] * r[3]);
    q[7] = 0.5f * ((t[0] * r[2] + t[2] * r[0]) - t[1] * r[1]);
}
// What pyr_scene_skin takes for a rotation in a dual-quaternion skin's joint: columns of length 1 and pairwise orthogonal within
// 1e-3, right-handed.
PYR_POSE_HD bool joint_is_rotation(const float* m) {
    const float *c0 = m, *c1 = m + 4, *c2 = m + 8;
    const auto dot = [](const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    if (!(magnitude(dot(c0, c0) - 1.0f) <= 1.0e-3f) || !(magnitude(dot(c1, c1) - 1.0f) <= 1.0e-3f) || !(magnitude(dot(c2, c2) - 1.0f) <= 1.0e-3f)) return false;
    if (!(magnitude(dot(c0, c1)) <= 1.0e-3f) || !(magnitude(dot(c0, c2)) <= 1.0e-3f) || !(magnitude(dot(c1, c2)) <= 1.0e-3f)) return false;
    float x[3];
    cross(c0, c1, x);
    return dot(x, c2) > 0.0f;
}
// One vertex's matrix from four joints' dual quaternions, `table` holding eight floats a joint and j0..j3 already compared against
// the skin's joint count. The pivot is joint j0: a joint whose rotation lies in the other hemisphere (dot4 < 0; zero or NaN does
// not) has its weight negated, so that q and -q, the same motion, blend the short way. Every entry of the blend is
// ((w0'*Q0 + w1'*Q1) + w2'*Q2) + w3'*Q3, unfused; it is normalised by its rotation part, t = 2 * (d * conj(r)) is the translation
// and cgmath's Matrix3::from(Quaternion) the upper 3x3; the last row is 0,0,0,1. The vertex then takes the per-vertex rule above
// with Pose{B, 1.0f, not identity}, exactly as after blend_joints. Returns whether the squared length that is normalised lies
// outside [1e-30, 1e30] (kBlendedRotation; what is written then is not used).
PYR_POSE_HD bool blend_dual_quaternions(const float* table, const uint32_t* j, const float* w, Pose& b) {
    const float *q0 = PYR_POSE_ROW16(table + 8 * (size_t)j[0]), *q1 = PYR_POSE_ROW16(table + 8 * (size_t)j[1]), *q2 = PYR_POSE_ROW16(table + 8 * (size_t)j[2]),
                *q3 = PYR_POSE_ROW16(table + 8 * (size_t)j[3]);
    const float w1 = dot4(q0, q1) < 0.0f ? -w[1] : w[1], w2 = dot4(q0, q2) < 0.0f ? -w[2] : w[2], w3 = dot4(q0, q3) < 0.0f ? -w[3] : w[3];
    float e[8];
    for (int i = 0; i < 8; ++i) e[i] = ((w[0] * q0[i] + w1 * q1[i]) + w2 * q2[i]) + w3 * q3[i];
    const float s = dot4(e, e);
    const bool bad = !(s >= 1.0e-30f && s <= 1.0e30f);
    const float k = reciprocal(root(s));
    const float r0 = e[0] * k, r1 = e[1] * k, r2 = e[2] * k, r3 = e[3] * k, d0 = e[4] * k, d1 = e[5] * k, d2 = e[6] * k, d3 = e[7] * k;
    const float x2 = r1 + r1, y2 = r2 + r2, z2 = r3 + r3;
    const float xx2 = x2 * r1, xy2 = x2 * r2, xz2 = x2 * r3, yy2 = y2 * r2, yz2 = y2 * r3, zz2 = z2 * r3, sx2 = x2 * r0, sy2 = y2 * r0, sz2 = z2 * r0;
    b.m[0] = 1.0f - yy2 - zz2, b.m[1] = xy2 + sz2, b.m[2] = xz2 - sy2, b.m[3] = 0.0f;
    b.m[4] = xy2 - sz2, b.m[5] = 1.0f - xx2 - zz2, b.m[6] = yz2 + sx2, b.m[7] = 0.0f;
    b.m[8] = xz2 + sy2, b.m[9] = yz2 - sx2, b.m[10] = 1.0f - xx2 - yy2, b.m[11] = 0.0f;
    b.m[12] = 2.0f * (((d1 * r0 - d0 * r1) - d2 * r3) + d3 * r2);
    b.m[13] = 2.0f * (((d2 * r0 - d0 * r2) + d1 * r3) - d3 * r1);
    b.m[14] = 2.0f * (((d3 * r0 - d0 * r3) - d1 * r2) + d2 * r1);
    b.m[15] = 1.0f;
    b.scale = 1.0f;
    b.identity = 0u;
    return bad;
}

// ---- the morph rule: what a vertex normal and its tangent frame become once the active targets' normal
// deltas have been added to the normal (`n` comes in as m = n + sum w[t] * dn[t], the caller's loop over the active targets in
// ascending t, and leaves as normalize(m)). `frame` nullptr: the scene keeps none; otherwise the old tangent frame is
// Gram-Schmidt'ed against the new normal, x first, which keeps it orthonormal and its handedness. Returns whether a squared
// length that is normalised lies outside [1e-30, 1e30] -- the range in which sqrt32 and rcp32 are the host's bits (exact_math.h);
// the caller raises its Flag bit then, and what is written is not used.
PYR_POSE_HD bool morph_normal_frame(float* n, float* frame) {
    const auto outside = [](float s) { return !(s >= 1.0e-30f && s <= 1.0e30f); };
    bool bad = outside((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    normalize(n);
    if (!frame) return bad;
    const float ex[3] = {1.0f, 0.0f, 0.0f}, ey[3] = {0.0f, 1.0f, 0.0f};
    float rx[3], ry[3], x[3], y[3];
    quat_rotate(frame, ex, rx);
    quat_rotate(frame, ey, ry);
    const float d = (rx[0] * n[0] + rx[1] * n[1]) + rx[2] * n[2];
    for (int a = 0; a < 3; ++a) x[a] = rx[a] - n[a] * d;
    bad = bad || outside((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    normalize(x);
    const float e = (ry[0] * n[0] + ry[1] * n[1]) + ry[2] * n[2];
    const float f = (ry[0] * x[0] + ry[1] * x[1]) + ry[2] * x[2];
    for (int a = 0; a < 3; ++a) y[a] = (ry[a] - n[a] * e) - x[a] * f;
    bad = bad || outside((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
    normalize(y);
    quat_from_cols(x, y, n, frame);
    return bad;
}

// ---- the smoothing rule: a vertex normal recomputed from where the surface is, as the sum of the face
// vectors of the triangles that share the vertex. A face vector is cross(p1 - p0, p2 - p0) -- twice the triangle's area along its
// geometric normal, so the sum is area-weighted -- and a triangle wound against its rest normals has its face vector negated:
// face_negated decides that once, from the rest pose (d of zero or NaN does not negate). The caller sums a group's face vectors
// in ascending corner order, starting from the first one (not from zero: 0 + (-0) loses a sign bit), and hands the sum to
// morph_normal_frame above, which normalises it, rebuilds the corner's tangent frame against it and range-checks what it
// normalises (kSmoothedNormal here).
PYR_POSE_HD void face_vector(const float* p, float* c) {
    const float a[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, b[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    cross(a, b, c);
}
PYR_POSE_HD bool face_negated(const float* rest_p, const float* rest_n) {
    float c[3];
    face_vector(rest_p, c);
    const float r[3] = {(rest_n[0] + rest_n[3]) + rest_n[6], (rest_n[1] + rest_n[4]) + rest_n[7], (rest_n[2] + rest_n[5]) + rest_n[8]};
    const float d = (c[0] * r[0] + c[1] * r[1]) + c[2] * r[2];
    return d < 0.0f;
}
PYR_POSE_HD void signed_face_vector(const float* p, bool negated, float* c) {
    face_vector(p, c);
    if (negated) c[0] = -c[0], c[1] = -c[1], c[2] = -c[2];
}

// ---- one lane's walk: what the kernels' lanes and the host rehearsal both call
// One vertex under one pose: an identity pose copies bits; the normal takes its frame along where the scene keeps frames.
PYR_POSE_HD void pose_vertex(const Pose& pose, float* p, float* n, float* frame, bool has_frames) {
    if (pose.identity) return;
    pose_point(pose, p);
    if (has_frames)
        pose_normal_frame(pose, n, frame);
    else
        pose_normal(pose, n);
}
// One skinned vertex: the skin first (a skin at rest copies), then the object's pose. `joints`: the skin's rows of the joint
// table; `j`: the four indices of the binding, relative to it. An index at or above the skin's count uses joint 0 and raises
// kBeyondRange (pyr_scene_set_skins has refused such a binding). Returns the bits raised.
PYR_POSE_HD uint32_t skin_vertex(const float* joints, uint32_t num_joints, bool skin_at_rest, const uint32_t* j, const float* w, const Pose& pose, float* p, float* n,
                                 float* frame, bool has_frames) {
    uint32_t raised = 0u;
    if (!skin_at_rest) {
        uint32_t inside[4];
        for (int k = 0; k < 4; ++k) {
            inside[k] = j[k];
            if (inside[k] >= num_joints) inside[k] = 0u, raised = kBeyondRange;
        }
        Pose blended;
        blend_joints(joints, inside, w, blended);
        pose_vertex(blended, p, n, frame, has_frames);
    }
    pose_vertex(pose, p, n, frame, has_frames);
    return raised;
}
// One vertex of a dual-quaternion skin: skin_vertex with blend_dual_quaternions in place of blend_joints.
// `table`: the skin's rows of the dual quaternion table. Returns the bits raised: kBeyondRange as there, kBlendedRotation.
PYR_POSE_HD uint32_t skin_vertex_dual(const float* table, uint32_t num_joints, bool skin_at_rest, const uint32_t* j, const float* w, const Pose& pose, float* p, float* n,
                                      float* frame, bool has_frames) {
    uint32_t raised = 0u;
    if (!skin_at_rest) {
        uint32_t inside[4];
        for (int k = 0; k < 4; ++k) {
            inside[k] = j[k];
            if (inside[k] >= num_joints) inside[k] = 0u, raised = kBeyondRange;
        }
        Pose blended;
        if (blend_dual_quaternions(table, inside, w, blended)) raised |= kBlendedRotation;
        pose_vertex(blended, p, n, frame, has_frames);
    }
    pose_vertex(pose, p, n, frame, has_frames);
    return raised;
}
// One active target's deltas added to `count` floats of a morphed triangle: x += w * d, unfused, the caller walking the active
// targets in ascending order. A morph with no active target adds nothing and so copies rest.
PYR_POSE_HD void add_delta(float* x, float w, const float* d, int count) {
    for (int k = 0; k < count; ++k) x[k] = x[k] + w * d[k];
}
// Whether a morph moves its normals at all (otherwise normals and frames are copied from rest), and one morphed vertex's normal
// finished once its deltas are in. Returns the bits raised.
PYR_POSE_HD bool morph_moves_normals(uint32_t has_normals, uint32_t num_active) { return has_normals != 0u && num_active != 0u; }
PYR_POSE_HD uint32_t morphed_normal(float* n, float* frame, bool has_frames) { return morph_normal_frame(n, has_frames ? frame : nullptr) ? kMorphedNormal : 0u; }
// One face added to a group's sum, from the triangle's nine final positions: the sum starts from the first face vector (`any`
// says whether there was one). And one corner finished from the sum: its normal and, where the scene keeps frames, its frame
// rebuilt against it. Returns the bits raised.
PYR_POSE_HD void add_face(const float* p, bool negated, float* sum, bool& any) {
    float f[3];
    signed_face_vector(p, negated, f);
    if (any)
        sum[0] = sum[0] + f[0], sum[1] = sum[1] + f[1], sum[2] = sum[2] + f[2];
    else
        sum[0] = f[0], sum[1] = f[1], sum[2] = f[2], any = true;
}
PYR_POSE_HD uint32_t finish_corner(const float* sum, float* n, float* frame, bool has_frames) {
    n[0] = sum[0], n[1] = sum[1], n[2] = sum[2];
    return morph_normal_frame(n, has_frames ? frame : nullptr) ? kSmoothedNormal : 0u;
}
// One sphere under one pose: radius *= scale; centre *= scale; centre = transform_point(centre)
PYR_POSE_HD void pose_sphere(const Pose& pose, float* s) {
    if (pose.identity) return;
    s[3] = s[3] * pose.scale;
    pose_point(pose, s);
}
// creation's coordinate check on a moved primitive's box (bvh_level.h triangle_bounds / sphere_bounds). Returns the bits raised.
PYR_POSE_HD uint32_t bounds_flag(const float* lo, const float* hi) {
    bool bad = false;
    for (int a = 0; a < 3; ++a) bad = bad || beyond_range(lo[a]) || beyond_range(hi[a]);
    return bad ? kBeyondRange : 0u;
}

// ---- the lamp rule: what a shape lamp's record takes from its shape, with pack_lamp's arithmetic (scene_pack.cpp)
struct LampShape {
    float v[3], width; // sphere: centre and radius
    float p[9], n[9];  // triangle: vertices and vertex normals
    float area;        // Shape::surface_area, unfused f32
};
PYR_POSE_HD void lamp_of_sphere(const float* s, LampShape& o) {
    o.v[0] = s[0], o.v[1] = s[1], o.v[2] = s[2];
    o.width = s[3];
    o.area = s[3] * s[3] * 4.0f * 3.14159265358979323846f;
}
PYR_POSE_HD void lamp_of_triangle(const float* p, const float* n, LampShape& o) {
    for (int k = 0; k < 9; ++k) o.p[k] = p[k], o.n[k] = n[k];
    const float a[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, b[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    float c[3];
    cross(a, b, c); // 0.5 * |a x b|
    o.area = 0.5f * root((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
}

} // namespace pose
} // namespace pyr
