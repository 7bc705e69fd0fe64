// Which instantiation of the throughput walk (kernels_hnsw.hip) a launch takes: the generic one, which reads the
// graph's shape from GraphTables at run time, or one with the shape compiled in (hnsw_walk_kernel's D and MAXM).
// Plain host arithmetic, shared by launch_coarse and tests/cpp/walk_shape_tool.cpp.
#pragma once

namespace ivfhnsw_gpu_impl {

struct WalkShape {
    int d;    // 128 or 96; 0 = the generic form
    int maxM; // 32; 0 = the generic form
};

// fmode, tagw, nch: what launch_coarse derived for this launch (rejection-filter form, visited-set tag width,
// 64-entry registers of the result set).  shape_on: the IVFHNSW_WALK_SHAPE knob (0 forces the generic form).
// The shaped forms exist for the neighbour-row filter (fmode 2 and 3) with the LDS visited set (tagw != 0), result sets
// of up to 128 entries (nch <= 2), 32 links per node in one 32-row record, and the two row lengths whose query share
// lives in registers (128: SIFT, 96: DEEP).  Everything else is the generic form.
inline WalkShape walk_shape_for(int d, int maxM, int nb_rows, int fmode, int tagw, int nch, bool shape_on)
{
    const WalkShape generic = {0, 0};
    if (!shape_on || (fmode != 2 && fmode != 3) || tagw == 0 || nch < 1 || nch > 2)
        return generic;
    if (maxM != 32 || nb_rows != 32 || (d != 128 && d != 96))
        return generic;
    const WalkShape s = {d, 32};
    return s;
}

} // namespace ivfhnsw_gpu_impl
