// mmw_summary.hpp -- the per-track output fields that mmw_track_summary (k_table<SITE>, k_misc.hip) and mmw_track_report
// (k_report_write, k_report.hip) share, computed in ONE place: a report row equals the table row of its (scene, slot) bit for bit
// because both are this function's.
#pragma once

#include "mmw_device.hpp"

namespace mmw {

// Row: mmw_track_summary or mmw_track_report (global memory or LDS: the stores follow the pointer).  rec == nullptr: a list
// position beyond the scene's tracks -- zeros.  The window / monitoring point (m_x .. fade_weight) are the context's or the scene's
// own site; everything arrives as scalars, so that the plain kernel (k_table<false>) reads its arguments exactly as it always did.
template <typename Row>
__device__ __forceinline__ void summary_fields(Row *o, const TrackRec *rec, int dx, double m_x, double m_y, double m_z, double fade_max,
                                               double fade_min, double fade_weight)
{
    const bool alive = rec != nullptr;
    o->point_num = alive ? rec->point_num : 0;
    o->lifetime = alive ? (float)rec->lifetime : 0.f;
    for (int e = 0; e < 9; e++) o->x[e] = (alive && e < dx) ? (float)rec->x[e] : 0.f;
    for (int e = 0; e < 6; e++) o->centroid[e] = alive ? (float)rec->centroid[e] : 0.f;
    for (int e = 0; e < MMW_NKP; e++) o->keypoints[e] = alive ? rec->kp[e] : 0.f;
    // calc_fade_square (Visualizer.py:14-29) over calc_projection_points (Utils.py:180-219), in the reference's
    // operation order, fp64 with the float32 keypoints widened (numpy 1.26, the reference's pinned version)
    double px = 0, pz = 0, size = 0;
    if (alive) {
        const double xo = rec->x[0] + (double)rec->kp[3], yo = rec->x[1] + (double)rec->kp[41], zo = (double)rec->kp[22];
        const double xd = xo - m_x, yd = yo - m_y, zd = zo - m_z;
        px = xd == 0 ? xo : -m_y / (yd / xd) + m_x;
        pz = zd == 0 ? zo : -m_y / (yd / zd) + m_z;
        const double sz = fade_max - (rec->x[1] + (double)rec->kp[12]) * fade_weight;
        size = fmax(fade_min, fmin(fade_max, sz));
    }
    o->fade_x = (float)px;
    o->fade_z = (float)pz;
    o->fade_size = (float)size;
}

}  // namespace mmw
