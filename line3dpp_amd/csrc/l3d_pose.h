// l3d_pose.h -- the pose state of DESIGN §27 that the refinement of camera poses (l3d_pose.hip) and the joint bundle of
// cameras and lines share: the delta (q, tau) on a camera's input pose about the model's
// centre, its update by a step (omega, tau), the camera as it is handed out and the closed form of K^-T.  Host only; fp64
// in the order §27 writes it.
#pragma once
#include <cmath>

#include "l3d_ctx.h"

namespace l3d {

// the delta (q, tau) on the input pose, t'_in = t_in + R_in c, and whether a step has been applied
struct PoseDelta {
    double q[4] = {1.0, 0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0}, tin[3] = {0.0, 0.0, 0.0};
    bool updated = false;
};

// R = R(q^) R_in and t' = R(q^) t'_in + tau: the pose in the frame about c
inline void pose_about_centre(const l3d_camera& in, const PoseDelta& s, double R[9], double tc[3]) {
    double qh[4] = {s.q[0], s.q[1], s.q[2], s.q[3]}, Rd[9];
    quat_normalise(qh);
    sim_rotation(qh, Rd);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (Rd[3 * i] * in.R[j] + Rd[3 * i + 1] * in.R[3 + j]) + Rd[3 * i + 2] * in.R[6 + j];
    const d3 u = mul33(Rd, d3{s.tin[0], s.tin[1], s.tin[2]});
    tc[0] = u.x + s.tau[0]; tc[1] = u.y + s.tau[1]; tc[2] = u.z + s.tau[2];
}

// the camera as it is handed out: the input, bit for bit, while no update has been made; else K, R and t = t' - R c
inline l3d_camera pose_camera_now(const l3d_camera& in, const PoseDelta& s, const double c[3]) {
    if (!s.updated) return in;
    l3d_camera out = in;
    double tc[3];
    pose_about_centre(in, s, out.R, tc);
    const d3 rc = mul33(out.R, d3{c[0], c[1], c[2]});
    out.t[0] = tc[0] - rc.x; out.t[1] = tc[1] - rc.y; out.t[2] = tc[2] - rc.z;
    return out;
}

// step 5's update of the delta: q <- dq (x) q, normalised (quat_step of l3d_dev.h, the alignment's); tau <- dR tau + delta_3..5
inline void pose_update(PoseDelta& s, const double delta[6]) {
    double dR[9];
    quat_step(delta, s.q, dR);
    const d3 u = mul33(dR, d3{s.tau[0], s.tau[1], s.tau[2]});
    s.tau[0] = u.x + delta[3]; s.tau[1] = u.y + delta[4]; s.tau[2] = u.z + delta[5];
    s.updated = true;
}

// the entries m00, m10, m11, m20, m21 of K^-T for an upper-triangular K with K22 = 1
inline void pose_inverse_transpose(const double* K, double M[5]) {
    M[0] = 1.0 / K[0];
    M[2] = 1.0 / K[4];
    M[1] = -((K[1] * M[0]) * M[2]);
    M[3] = -(K[2] * M[0]) - K[5] * M[1];
    M[4] = -(K[5] * M[2]);
}

}  // namespace l3d
