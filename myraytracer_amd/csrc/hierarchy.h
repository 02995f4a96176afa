// The host-side hierarchy builder (hierarchy.cpp): clusters, upper levels, boxes and the matrix-core sweep's operand of a scene,
// as mrt_set_world_raw (world.cpp) uploads them.  Pure host code.  Internal: not installed.
#pragma once
#include <vector>

#include "bounds.h"

namespace mrt {

// Upper levels of the hierarchy: level k+1 bounds 4 consecutive level-k nodes (consecutive in kd order,
// so neighbours in space); its bounding sphere is measured from the MEMBER spheres under
// it, R = kBoundInflate x the enclosing radius from the f32-rounded centre, so the conservativeness argument of
// the clusters holds for every level.  Levels are added while the top has more than
// top_target records (the sweep costs every ray one test per top record; a walk round costs about 1.5
// wave-instructions per item).  Every level is padded to a multiple of 4 (the top: kGroup) with
// never-hit records; the children of a never-hit node are never read.
struct Hierarchy {
    std::vector<mrt::SphereRec> top, nodes;
    std::vector<uint32_t> member_index;
    std::vector<mrt::BoxFull> boxes;          // levels 1 .. levels (the top last), level k at box_base[k]
    uint32_t box_base[mrt::kMaxLevels + 1] = {0, 0, 0, 0, 0};
    bool box_quad = false;
    float box_kc = 0.0f;                      // the slack's coefficient of X: one per scene
    uint32_t levels = 1, n_members = 0;       // n_members: level 0 including the direct spheres
    uint32_t level_base[mrt::kMaxLevels] = {0, 0, 0, 0};
    uint32_t n_direct = 0, direct_first = 0;
    uint32_t n_pool = 0;                      // the clusters [0, n_pool) are those build_clusters made from its pool (regroup.hip)
    mrt::SphereRec direct[mrt::kMaxDirect] = {};
    uint32_t direct_index[mrt::kMaxDirect] = {};
};

// the hierarchy of n spheres (centers4: 4 floats each); its boxes in the kernel's top-down numbering (KParams::boxes) and in the form
// the kernel reads; its top level as the matrix-core sweep's A operand; KParams::mfma_scale / mfma_neg_k2_pair for rays and
// records within `all` of the sweep's origin
void build_hierarchy(const float* centers4, const float* radii, uint32_t n, float factor, uint32_t max_levels,
                     uint32_t top_target, Hierarchy& H);
void boxes_top_down(const Hierarchy& H, bool open, std::vector<BoxFull>& out, uint32_t* cluster_first, uint32_t* cluster_parent_first);
void pack_boxes(const std::vector<BoxFull>& full, std::vector<BoxRec>& out);
void build_top_mfma(const std::vector<SphereRec>& top, std::vector<uint16_t>& out, float origin[3], double* max_c2,
                    double* med_r2, size_t* n_real);
void mfma_scales(double all, float scale[4], uint32_t* neg_k2_pair);
// The space the matrix-core sweep of a scene runs in: x' = D (x - origin), D = diag(axis) with entries 1, 2 or 4 chosen from
// the spheres alone (`force`: a caller's D instead), and the A operand of the top level's bounds in that space -- for D = I
// exactly what build_top_mfma gives.  rel_out: those bounds as records.  sweep_reach: how far the spheres reach there.
void build_sweep_operand(const Hierarchy& H, const float* force, float axis[3], std::vector<uint16_t>& out, float origin[3],
                         double* max_c2, double* med_r2, size_t* n_real, std::vector<SphereRec>* rel_out);
double sweep_reach(const float* centers4, const float* radii, uint32_t n, const float origin[3], const float axis[3]);

}  // namespace mrt
