// The host-side hierarchy builder: what mrt_set_world_raw (world.cpp) uploads for a scene besides the spheres themselves -- the
// clusters, the upper levels, the boxes of large scenes, the matrix-core sweep's operand -- and the host-only diagnostics over
// them.  Nothing here calls into the GPU runtime.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>

#include "hierarchy.h"

namespace mrt {

namespace {

// Clusters.  The kernel's sweep does not need the spheres themselves, only a conservative "could this
// ray touch it" test, so spatially close spheres are tested in CLUSTERS of up to kClusterK through one
// bounding sphere and the per-sphere discriminants are evaluated only for the members of the few clusters
// that pass.  A ray's expected number of candidates is proportional to the sum of the bounds' cross
// sections, so the grouping minimises sum(R^2): spheres are split kd-tree fashion (widest axis of the
// centres, at a multiple of kClusterK near the median) down to groups of <= 8, and such a group is cut
// into 4 + rest by trying every choice.  Spheres far larger than the median (a ground sphere) stay alone;
// factor == 0 (diagnostic) gives every sphere a cluster of its own.  Consecutive clusters are kd siblings, which is what
// the upper levels (build_hierarchy) group.  The bounds are bounds.h's (Span, bound_record).  Clusters are padded to
// kClusterK members and the list to a multiple of kGroup with never-hit records (-r^2 = +inf gives a
// discriminant of -inf).
void build_clusters(const float* centers4, const float* radii, uint32_t n, float factor,
                    std::vector<mrt::SphereRec>& clusters, std::vector<mrt::SphereRec>& members,
                    std::vector<uint32_t>& member_index, std::vector<uint32_t>& direct, uint32_t* n_pool) {
    clusters.clear(); members.clear(); member_index.clear(); direct.clear();
    const mrt::SphereRec never = never_hit_record();
    std::vector<double> rs(n);
    for (uint32_t i = 0; i < n; i++) rs[i] = std::fabs((double)radii[i]);
    double big = 1e300;
    if (n > 1) {
        std::vector<double> sorted = rs;
        std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
        big = 8.0 * sorted[n / 2];
    }
    // enclosing sphere of a set (bounds.h, Span): R, and the f32-rounded centre it is measured from
    auto enclose = [&](const uint32_t* idx, uint32_t cnt, float ctr[3]) -> double {
        Span s;
        for (uint32_t m = 0; m < cnt; m++) s.add(centers4 + 4 * idx[m], rs[idx[m]]);
        s.centre(ctr);
        double R = 0;
        for (uint32_t m = 0; m < cnt; m++) R = std::max(R, reach_from(ctr, centers4 + 4 * idx[m], rs[idx[m]]));
        return R;
    };
    std::vector<std::vector<uint32_t>> groups;
    std::vector<uint32_t> pool;                      // spheres that may share a cluster
    std::vector<uint32_t> alone;
    for (uint32_t i = 0; i < n; i++) (factor > 0.0f && rs[i] <= big ? pool : alone).push_back(i);
    // iterative kd split of pool[lo, hi)
    std::vector<std::pair<uint32_t, uint32_t>> stack;
    if (!pool.empty()) stack.push_back({0u, (uint32_t)pool.size()});
    std::vector<std::pair<uint32_t, uint32_t>> leaves;      // in kd order
    while (!stack.empty()) {
        const auto [lo, hi] = stack.back();
        stack.pop_back();
        const uint32_t m = hi - lo;
        if (m <= 2 * mrt::kClusterK) { leaves.push_back({lo, hi}); continue; }
        double bl[3] = {1e300, 1e300, 1e300}, bh[3] = {-1e300, -1e300, -1e300};
        for (uint32_t q = lo; q < hi; q++)
            for (int k = 0; k < 3; k++) {
                bl[k] = std::min(bl[k], (double)centers4[4 * pool[q] + k]);
                bh[k] = std::max(bh[k], (double)centers4[4 * pool[q] + k]);
            }
        int ax = 0;
        for (int k = 1; k < 3; k++) if (bh[k] - bl[k] > bh[ax] - bl[ax]) ax = k;
        std::stable_sort(pool.begin() + lo, pool.begin() + hi, [&](uint32_t x, uint32_t y) {
            const float cx = centers4[4 * x + ax], cy = centers4[4 * y + ax];
            return cx < cy || (cx == cy && x < y);
        });
        uint32_t h = (m / 2 + mrt::kClusterK - 1) / mrt::kClusterK * mrt::kClusterK;
        if (h >= m) h = m - mrt::kClusterK;
        stack.push_back({lo + h, hi});              // popped second: keeps the leaves in left-to-right order
        stack.push_back({lo, lo + h});
    }
    for (const auto& [lo, hi] : leaves) {
        const uint32_t m = hi - lo;
        if (m <= mrt::kClusterK) { groups.emplace_back(pool.begin() + lo, pool.begin() + hi); continue; }
        // 5..8 spheres: the first one plus the 3 others that minimise R_A^2 + R_B^2
        uint32_t bestmask = 0;
        double best = 1e300;
        for (uint32_t mask = 0; mask < (1u << m); mask++) {
            if (!(mask & 1u) || __builtin_popcount(mask) != (int)mrt::kClusterK) continue;
            uint32_t A[8], B[8], na = 0, nb = 0;
            for (uint32_t q = 0; q < m; q++) ((mask >> q) & 1u ? A[na++] : B[nb++]) = pool[lo + q];
            float ctr[3];
            const double ra = enclose(A, na, ctr), rb = enclose(B, nb, ctr);
            if (ra * ra + rb * rb < best) { best = ra * ra + rb * rb; bestmask = mask; }
        }
        std::vector<uint32_t> A, B;
        for (uint32_t q = 0; q < m; q++) ((bestmask >> q) & 1u ? A : B).push_back(pool[lo + q]);
        groups.push_back(A);
        groups.push_back(B);
    }
    // Refinement: swap one member between two clusters whose bounds overlap (or move one into a cluster
    // with a free slot) whenever that lowers R_a^2 + R_b^2, until nothing improves (C3: sum R^2 185 -> 175).
    // Every pair for up to 4,096 clusters, otherwise the 32 following clusters in kd order.
    {
        const size_t ng = groups.size();
        std::vector<double> gr(ng);
        std::vector<std::array<double, 3>> gc(ng);
        auto refresh = [&](size_t g) { float c3[3]; gr[g] = enclose(groups[g].data(), (uint32_t)groups[g].size(), c3); gc[g] = {c3[0], c3[1], c3[2]}; };
        for (size_t g = 0; g < ng; g++) refresh(g);
        const size_t window = ng <= 4096 ? ng : 32;
        for (int pass = 0; pass < (ng <= 4096 ? 4 : 2); pass++) {
            size_t improved = 0;
            for (size_t a = 0; a < ng; a++) {
                for (size_t b = a + 1; b < ng && b <= a + window; b++) {
                    double d2 = 0;
                    for (int k = 0; k < 3; k++) d2 += (gc[a][k] - gc[b][k]) * (gc[a][k] - gc[b][k]);
                    if (d2 > (gr[a] + gr[b]) * (gr[a] + gr[b])) continue;
                    const double base = gr[a] * gr[a] + gr[b] * gr[b];
                    double best = base - 1e-12 * base;
                    std::vector<uint32_t> bestA, bestB;
                    std::vector<uint32_t> A, B;
                    float c3[3];
                    auto consider = [&]() {
                        const double ra = enclose(A.data(), (uint32_t)A.size(), c3), rb = enclose(B.data(), (uint32_t)B.size(), c3);
                        if (ra * ra + rb * rb < best) { best = ra * ra + rb * rb; bestA = A; bestB = B; }
                    };
                    for (size_t i = 0; i < groups[a].size(); i++)
                        for (size_t j = 0; j < groups[b].size(); j++) {
                            A = groups[a]; B = groups[b];
                            std::swap(A[i], B[j]);
                            consider();
                        }
                    if (groups[b].size() < mrt::kClusterK && groups[a].size() > 1)
                        for (size_t i = 0; i < groups[a].size(); i++) {
                            A = groups[a]; B = groups[b];
                            B.push_back(A[i]); A.erase(A.begin() + (long)i);
                            consider();
                        }
                    if (groups[a].size() < mrt::kClusterK && groups[b].size() > 1)
                        for (size_t j = 0; j < groups[b].size(); j++) {
                            A = groups[a]; B = groups[b];
                            A.push_back(B[j]); B.erase(B.begin() + (long)j);
                            consider();
                        }
                    if (!bestA.empty()) {
                        groups[a] = bestA; groups[b] = bestB;
                        refresh(a); refresh(b);
                        improved++;
                    }
                }
            }
            if (!improved) break;
        }
    }
    *n_pool = (uint32_t)groups.size();               // the clusters made from `pool` come first (regroup.hip permutes over them)
    // the largest of the big spheres are tested by every ray directly (KParams::direct); the others get a
    // cluster of their own
    std::stable_sort(alone.begin(), alone.end(), [&](uint32_t x, uint32_t y) { return rs[x] > rs[y]; });
    for (uint32_t q = 0; q < alone.size(); q++) {
        if (factor > 0.0f && q < mrt::kMaxDirect && rs[alone[q]] > big) direct.push_back(alone[q]);
        else groups.push_back({alone[q]});
    }
    for (auto& g : groups) {
        std::sort(g.begin(), g.end());
        float ctr[3];
        const double R = enclose(g.data(), (uint32_t)g.size(), ctr);
        clusters.push_back(bound_record(ctr, R));
        for (uint32_t m = 0; m < mrt::kClusterK; m++) {
            if (m < g.size()) {
                const float r = radii[g[m]];
                members.push_back(mrt::SphereRec{centers4[4 * g[m]], centers4[4 * g[m] + 1], centers4[4 * g[m] + 2], -(r * r)});
                member_index.push_back(g[m]);
            } else {
                members.push_back(never);
                member_index.push_back(0u);
            }
        }
    }
    while (clusters.empty() || clusters.size() % mrt::kGroup != 0) {
        clusters.push_back(never);                                    // S = -inf: never a candidate
        for (uint32_t m = 0; m < mrt::kClusterK; m++) { members.push_back(never); member_index.push_back(0u); }
    }
}

// The spheres in the member slots [j span, (j+1) span) of the hierarchy part of level 0 -- what node j of a level bounds:
// f(centre, |radius|) for each.  Never-hit padding slots are skipped.
template <class F>
void for_members_under(const float* centers4, const float* radii, const std::vector<mrt::SphereRec>& members,
                       const std::vector<uint32_t>& member_index, size_t j, size_t span, F&& f) {
    for (size_t m = j * span, m1 = std::min(members.size(), (j + 1) * span); m < m1; m++)
        if (std::isfinite(members[m].neg_r2)) f(centers4 + 4 * member_index[m], std::fabs((double)radii[member_index[m]]));
}

// The boxes of every node (levels 1 .. top), for the walk of large scenes (sweep.h, box_may_touch): node j of level k covers the
// members [j 4^k, (j+1) 4^k).  The extents, the two forms of the slack K and their constants are bounds.h's (box_extents,
// box_kpad); here the scene takes the form that is smaller at its own reach, and its one kc.
void build_boxes(const float* centers4, const float* radii, const std::vector<mrt::SphereRec>& members, Hierarchy& H) {
    const mrt::BoxFull never_box{0.0f, 0.0f, 0.0f, kBoxNeverExtent, kBoxNeverExtent, kBoxNeverExtent, 0.0f, 0.0f};
    H.boxes.clear();
    // the scene's reach and smallest radius decide the form of the slack
    double lo_all[3] = {1e300, 1e300, 1e300}, hi_all[3] = {-1e300, -1e300, -1e300}, r_small = 1e300;
    for_members_under(centers4, radii, members, H.member_index, 0, members.size(), [&](const float* c, double r) {
        r_small = std::min(r_small, r);
        for (int k = 0; k < 3; k++) { lo_all[k] = std::min(lo_all[k], (double)c[k]); hi_all[k] = std::max(hi_all[k], (double)c[k]); }
    });
    double reach = 0.0;
    if (lo_all[0] <= hi_all[0]) {
        for (int k = 0; k < 3; k++) reach += (hi_all[k] - lo_all[k]) * (hi_all[k] - lo_all[k]);
        reach = std::sqrt(reach);
    }
    // (by the scene's SMALLEST radius, since kc is one value per scene: a scene with a few tiny spheres takes the linear form)
    H.box_quad = kBoxQuadKc / std::max(r_small, 1e-300) * reach < kBoxLinKc * 2.0;      // quadratic slack at the reach < 2 x the linear one
    const double kc_scene = H.box_quad ? quad_kc_for_radius(r_small) : kBoxLinKc;
    H.box_kc = H.box_quad ? round_up_f32(kc_scene) : (float)kBoxLinKc;
    for (uint32_t k = 1; k <= H.levels; k++) {
        H.box_base[k] = (uint32_t)H.boxes.size();
        const size_t n_k = k == H.levels ? H.top.size() : (size_t)((k + 1 < H.levels ? H.level_base[k + 1] : (uint32_t)H.nodes.size()) - H.level_base[k]);
        for (size_t j = 0; j < n_k; j++) {
            Span s;
            for_members_under(centers4, radii, members, H.member_index, j, (size_t)1 << (2 * k), [&](const float* c, double r) { s.add(c, r); });
            if (s.empty()) { H.boxes.push_back(never_box); continue; }
            const BoxExtents b = box_extents(s);
            H.boxes.push_back(mrt::BoxFull{b.c[0], b.c[1], b.c[2], b.e[0], b.e[1], b.e[2], H.box_kc, box_kpad(H.box_quad, (double)H.box_kc, kc_scene, b.e1, b.e2)});
        }
    }
}

}  // namespace

// What the kernel reads of a box (mrt_internal.h, BoxRec): the centre and the extents with kpad folded in (bounds.h, fold_kpad)
void pack_boxes(const std::vector<mrt::BoxFull>& full, std::vector<mrt::BoxRec>& out) {
    out.resize(full.size());
    for (size_t i = 0; i < full.size(); i++) {
        const mrt::BoxFull& b = full[i];
        const bool real = b.ex >= 0.0f && b.ex < 1.0e37f;           // (never-hit: kBoxNeverExtent; opened wide: kBoxOpenExtent)
        out[i] = real ? mrt::BoxRec{b.cx, b.cy, b.cz, fold_kpad(b.ex, b.kpad), fold_kpad(b.ey, b.kpad), fold_kpad(b.ez, b.kpad)}
                      : mrt::BoxRec{b.cx, b.cy, b.cz, b.ex, b.ey, b.ez};
    }
}

// The boxes in the order the kernel walks them (KParams::boxes): depth t of the hierarchy (0 = the swept top = level
// `levels`, levels - 1 = the clusters = level 1) at o_t = n_top (4^t - 1) / 3, n_top = the padded top: the children of node g
// are 4 g + n_top .. + 3 whatever its depth, so a work item needs no level.  Slots without a node hold never-hit boxes.
// `open`: every real box opened wide (kBoxOpenExtent: the test never rejects) -- the A/B form of mrt_debug_set_boxes(0).
void boxes_top_down(const Hierarchy& H, bool open, std::vector<mrt::BoxFull>& out, uint32_t* cluster_first, uint32_t* cluster_parent_first) {
    const mrt::BoxFull never_box{0.0f, 0.0f, 0.0f, kBoxNeverExtent, kBoxNeverExtent, kBoxNeverExtent, 0.0f, 0.0f};
    const size_t n_top = H.top.size();
    size_t o[mrt::kMaxLevels + 1];
    o[0] = 0;
    for (uint32_t t = 0; t < H.levels; t++) o[t + 1] = o[t] + (n_top << (2 * t));
    out.assign(o[H.levels], never_box);
    for (uint32_t t = 0; t < H.levels; t++) {
        const uint32_t k = H.levels - t;                 // the level at this depth
        const size_t first = H.box_base[k], last = k < H.levels ? H.box_base[k + 1] : H.boxes.size();
        for (size_t j = 0; j < last - first && j < (n_top << (2 * t)); j++) {
            mrt::BoxFull b = H.boxes[first + j];
            if (open && b.ex >= 0.0f) b.ex = b.ey = b.ez = kBoxOpenExtent;
            out[o[t] + j] = b;
        }
    }
    *cluster_first = (uint32_t)o[H.levels - 1];
    *cluster_parent_first = H.levels >= 2 ? (uint32_t)o[H.levels - 2] : 0u;
}

constexpr uint32_t kBoxMinMembers = 4096;     // member slots from which the walk tests boxes by default (fill_scene_params)
void build_hierarchy(const float* centers4, const float* radii, uint32_t n, float factor, uint32_t max_levels,
                     uint32_t top_target, Hierarchy& H) {
    const mrt::SphereRec never = never_hit_record();
    std::vector<mrt::SphereRec> members, cur;
    std::vector<uint32_t> direct;
    build_clusters(centers4, radii, n, factor, cur, members, H.member_index, direct, &H.n_pool);
    H.nodes = members;
    // the direct spheres follow the clusters' members in level 0 (no cluster, no bound above them)
    H.n_direct = (uint32_t)direct.size();
    H.direct_first = (uint32_t)members.size();
    for (uint32_t j = 0; j < mrt::kClusterK; j++) {
        mrt::SphereRec rec = never;
        uint32_t idx = 0;
        if (j < direct.size()) {
            idx = direct[j];
            const float r = radii[idx];
            rec = mrt::SphereRec{centers4[4 * idx], centers4[4 * idx + 1], centers4[4 * idx + 2], -(r * r)};
        }
        H.direct[j] = rec;
        H.direct_index[j] = idx;
        if (!direct.empty()) { H.nodes.push_back(rec); H.member_index.push_back(idx); }
    }
    static_assert(mrt::kMaxDirect == mrt::kClusterK, "level 0 stays a multiple of kClusterK");
    H.n_members = (uint32_t)H.nodes.size();
    H.levels = 1;
    H.level_base[0] = 0;
    // scenes whose members fit 10-bit ids (the kernel's SMALL variant) keep one level: with <= 256 clusters
    // the sweep is cheap and the bounds of 16 spheres are loose (C3: a ray touches 10 of 38 such bounds)
    if (scene_is_small(H.n_members)) max_levels = 1;
    // top_target 0 = automatic: levels are added while the top has more than 256 records -- 128 where the walk tests boxes
    // below the top, which make a smaller top cheaper (round 3: 4,901 spheres 34.1 -> 33.3 ms per 64-spp frame, 10,001 spheres
    // 48.2 -> 47.3; without boxes 1,297 / 2,501 spheres lose 20 % with a top of <= 64)
    if (top_target == 0) top_target = H.n_members > kBoxMinMembers ? 128u : 256u;
    while (H.levels < max_levels && cur.size() > top_target) {
        const size_t span = (size_t)1 << (2 * (H.levels + 1));        // members under one node of the new level
        const size_t n_par = (cur.size() + 3) / 4;
        std::vector<mrt::SphereRec> par;
        par.reserve(n_par + mrt::kGroup);
        for (size_t j = 0; j < n_par; j++) {
            Span s;
            for_members_under(centers4, radii, members, H.member_index, j, span, [&](const float* c, double r) { s.add(c, r); });
            if (s.empty()) { par.push_back(never); continue; }
            float ctr[3];
            s.centre(ctr);
            double R = 0;
            for_members_under(centers4, radii, members, H.member_index, j, span, [&](const float* c, double r) { R = std::max(R, reach_from(ctr, c, r)); });
            par.push_back(bound_record(ctr, R));
        }
        while (cur.size() % 4 != 0) cur.push_back(never);
        H.level_base[H.levels] = (uint32_t)H.nodes.size();
        H.nodes.insert(H.nodes.end(), cur.begin(), cur.end());
        cur.swap(par);
        H.levels++;
    }
    while (cur.empty() || cur.size() % 32 != 0) cur.push_back(never);      // 32 = one tile of the matrix-core sweep
    H.top.swap(cur);
    build_boxes(centers4, radii, members, H);
}

// the GEMMs of the matrix-core sweep run in coordinates relative to the centre of the records' bounding box (the slack grows
// with the squared distances from THAT point, wherever the scene sits); the kernel subtracts it from the ray origin
static void sweep_origin(const std::vector<mrt::SphereRec>& top, float origin[3]) {
    double lo[3] = {1e300, 1e300, 1e300}, hi3[3] = {-1e300, -1e300, -1e300};
    for (const auto& r : top) {
        if (!std::isfinite(r.neg_r2)) continue;
        const double c[3] = {r.cx, r.cy, r.cz};
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], c[k]); hi3[k] = std::max(hi3[k], c[k]); }
    }
    for (int k = 0; k < 3; k++) origin[k] = lo[k] <= hi3[k] ? (float)(0.5 * (lo[k] + hi3[k])) : 0.0f;
}

// The top level once more, as the A operand of the matrix-core sweep: the rows and their placement are bounds.h's (mfma_row).
// Also returns what set_world needs to decide whether the slack is negligible: the largest C.C and the median R^2.
// `rel`: the records relative to the sweep's origin, in the top level's order (build_top_mfma, build_sweep_operand).
static void pack_top_mfma(const std::vector<mrt::SphereRec>& rel, std::vector<uint16_t>& out, double* max_c2, double* med_r2, size_t* n_real) {
    const size_t tiles = rel.size() / 32;
    out.assign(tiles * 512, 0);
    std::vector<double> r2s;
    *max_c2 = 0.0;
    for (size_t t = 0; t < tiles; t++)
        for (uint32_t m = 0; m < 32; m++) {
            const mrt::SphereRec& r = rel[mfma_source_record((uint32_t)t, m)];
            if (std::isfinite(r.neg_r2)) {
                const MfmaTerms terms = mfma_terms(r);
                *max_c2 = std::max(*max_c2, terms.c2);
                r2s.push_back(terms.R2);
            }
            uint16_t row[16];
            mfma_row(r, row);
            for (uint32_t q = 0; q < 16; q++) out[t * 512 + mfma_slot(m, q)] = row[q];
        }
    *n_real = r2s.size();
    *med_r2 = 0.0;
    if (!r2s.empty()) { std::nth_element(r2s.begin(), r2s.begin() + r2s.size() / 2, r2s.end()); *med_r2 = r2s[r2s.size() / 2]; }
}

// the world-space top records relative to the origin (bounds.h, relative_record)
static void relative_records(const std::vector<mrt::SphereRec>& top, const float origin[3], std::vector<mrt::SphereRec>& rel) {
    rel.resize(top.size());
    for (size_t i = 0; i < top.size(); i++) rel[i] = relative_record(top[i], origin);
}

void build_top_mfma(const std::vector<mrt::SphereRec>& top, std::vector<uint16_t>& out, float origin[3], double* max_c2,
                    double* med_r2, size_t* n_real) {
    sweep_origin(top, origin);
    std::vector<mrt::SphereRec> rel;
    relative_records(top, origin, rel);
    pack_top_mfma(rel, out, max_c2, med_r2, n_real);
}

// The sweep's own space: x' = D (x - origin), D = diag(axis), every entry 1, 2 or 4.  A line that meets a
// member sphere meets, in that space, the scaled member -- an ellipsoid with the semi-axes r D -- hence any sphere that
// encloses the scaled members of its cluster, and flat clusters get much smaller spheres there.  rel[j] = such a sphere for
// top record j, from the member spheres under it: centre = centre of the scaled members' common box, rounded to f32; radius =
// bound_record of the largest distance from THAT point to a point of a scaled member.  That distance, max |p + r D u| over
// unit u, is the minimum over lambda > max (r D_k)^2 of lambda + sum_k p_k^2 lambda / (lambda - (r D_k)^2) (Lagrange
// dual; EVERY lambda gives an upper bound, so the search below cannot make the result too small), never above the two
// plain bounds |p| + r max D and |(|p_k| + r D_k)_k|.  Returns false where the proof of DESIGN.md §4 does not hold
// for this D: a line that the reference's rounded discriminant accepts passes a member of radius r by up to 7 eps |oc|^2 / r, which
// max D stretches; the direction's stretch pays for that only while max D E / r + (max D)^2 <= 36 (E the enclosing radius).
constexpr double kScaledMarginBudget = 36.0;
static bool scaled_top_records(const Hierarchy& H, const float axis[3], const float origin[3], std::vector<mrt::SphereRec>& rel) {
    const mrt::SphereRec never{0.0f, 0.0f, 0.0f, INFINITY};
    const size_t span = (size_t)1 << (2 * H.levels), n_hier = std::min((size_t)H.direct_first, H.nodes.size());
    const double D[3] = {axis[0], axis[1], axis[2]}, dmax = std::max(D[0], std::max(D[1], D[2]));
    rel.assign(H.top.size(), never);
    bool proven = true;
    for (size_t j = 0; j < H.top.size(); j++) {
        const size_t m0 = std::min(n_hier, j * span), m1 = std::min(n_hier, (j + 1) * span);
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, r_min = 1e300;
        for (size_t m = m0; m < m1; m++) {
            const mrt::SphereRec& s = H.nodes[m];
            if (!std::isfinite(s.neg_r2)) continue;
            const double r = std::sqrt(-(double)s.neg_r2) * (1.0 + 0x1p-22), c[3] = {s.cx, s.cy, s.cz};     // (-(r r) was rounded to f32)
            for (int k = 0; k < 3; k++) {
                const double ck = D[k] * (c[k] - origin[k]);
                lo[k] = std::min(lo[k], ck - r * D[k]);
                hi[k] = std::max(hi[k], ck + r * D[k]);
            }
            r_min = std::min(r_min, r);
        }
        if (!(lo[0] <= hi[0])) continue;
        float ctr[3];
        for (int k = 0; k < 3; k++) ctr[k] = (float)(0.5 * (lo[k] + hi[k]));
        double E = 0.0;
        for (size_t m = m0; m < m1; m++) {
            const mrt::SphereRec& s = H.nodes[m];
            if (!std::isfinite(s.neg_r2)) continue;
            const double r = std::sqrt(-(double)s.neg_r2) * (1.0 + 0x1p-22), c[3] = {s.cx, s.cy, s.cz};
            double p2[3], a2[3], pn = 0.0, box = 0.0, a2max = 0.0;
            for (int k = 0; k < 3; k++) {
                const double pk = D[k] * (c[k] - origin[k]) - (double)ctr[k], ak = r * D[k];
                p2[k] = pk * pk; a2[k] = ak * ak;
                pn += p2[k]; box += (std::fabs(pk) + ak) * (std::fabs(pk) + ak); a2max = std::max(a2max, a2[k]);
            }
            double best = std::min(std::sqrt(pn) + r * dmax, std::sqrt(box));
            best *= best;
            auto dual = [&](double x) {                   // lambda = a2max + x
                const double l = a2max + x;
                double v = l;
                for (int k = 0; k < 3; k++) v += p2[k] * l / (l - a2[k]);
                return v;
            };
            // convex in lambda: ternary search over x = lambda - a2max on a logarithmic axis
            double xl = std::log(1e-9 * (a2max + pn) + 1e-300), xh = std::log(4.0 * (a2max + pn) + 1e-300);
            for (int it = 0; it < 80; it++) {
                const double x1 = xl + (xh - xl) / 3.0, x2 = xh - (xh - xl) / 3.0;
                if (dual(std::exp(x1)) < dual(std::exp(x2))) xh = x2; else xl = x1;
            }
            const double v = dual(std::exp(0.5 * (xl + xh)));
            if (std::isfinite(v) && v < best) best = v;
            E = std::max(E, std::sqrt(best) * (1.0 + 1e-12));
        }
        if (!(r_min > 0.0) || dmax * E / r_min + dmax * dmax > kScaledMarginBudget) proven = false;
        rel[j] = bound_record(ctr, E);
    }
    return proven;
}

// D for a scene (mrt_set_world_raw): the candidates -- one axis scaled by 2 or by 4 -- are scored by how many bounds a fixed,
// seeded set of lines through the box of the clustered spheres meets (half of them through two points of the box, which
// favours the grazing directions a camera beside a flat scene produces; half through one point in a uniformly random
// direction, as scattered rays run), against the world-space records' count.  The set only steers the choice: any D is
// correct.  It depends on the spheres alone, never on the camera.  D = I unless the best candidate meets at least 5 % fewer
// bounds, its proof holds (scaled_top_records) and the sweep's give-away stays as negligible in its space as the scene test of
// mrt_set_world_raw demands.  One-level hierarchies only: the walk of larger scenes has its boxes.
static void choose_sweep_axes(const Hierarchy& H, const float origin[3], float axis[3]) {
    axis[0] = axis[1] = axis[2] = 1.0f;
    if (H.levels != 1) return;
    const size_t n_hier = std::min((size_t)H.direct_first, H.nodes.size());
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (size_t m = 0; m < n_hier; m++) {
        const mrt::SphereRec& s = H.nodes[m];
        if (!std::isfinite(s.neg_r2)) continue;
        const double r = std::sqrt(-(double)s.neg_r2), c[3] = {s.cx, s.cy, s.cz};
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], c[k] - r); hi[k] = std::max(hi[k], c[k] + r); }
    }
    if (!(lo[0] <= hi[0])) return;
    constexpr int kLines = 4096;
    std::vector<double> lines(6 * kLines);
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto uniform = [&]() {                              // splitmix64 -> [0, 1)
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (double)((z ^ (z >> 31)) >> 11) * 0x1p-53;
    };
    for (int i = 0; i < kLines; i++) {
        double* L = lines.data() + 6 * i;
        for (int k = 0; k < 3; k++) L[k] = lo[k] + uniform() * (hi[k] - lo[k]);
        if (i & 1) {
            for (int k = 0; k < 3; k++) L[3 + k] = lo[k] + uniform() * (hi[k] - lo[k]) - L[k];
        } else {
            const double z = 2.0 * uniform() - 1.0, phi = 6.283185307179586 * uniform(), q = std::sqrt(1.0 - z * z);
            L[3] = q * std::cos(phi); L[4] = q * std::sin(phi); L[5] = z;
        }
        if (L[3] * L[3] + L[4] * L[4] + L[5] * L[5] < 1e-300) L[3] = 1.0;
    }
    auto score = [&](const std::vector<mrt::SphereRec>& rel, const float ax[3]) {
        size_t met = 0;
        for (int i = 0; i < kLines; i++) {
            const double* L = lines.data() + 6 * i;
            double p[3], u[3], uu = 0.0;
            for (int k = 0; k < 3; k++) { p[k] = ax[k] * (L[k] - origin[k]); u[k] = ax[k] * L[3 + k]; uu += u[k] * u[k]; }
            for (const auto& r : rel) {
                if (!std::isfinite(r.neg_r2)) continue;
                const double w[3] = {p[0] - r.cx, p[1] - r.cy, p[2] - r.cz};
                const double b = w[0] * u[0] + w[1] * u[1] + w[2] * u[2];
                if (w[0] * w[0] + w[1] * w[1] + w[2] * w[2] - b * b / uu <= -(double)r.neg_r2) met++;
            }
        }
        return met;
    };
    std::vector<mrt::SphereRec> rel;
    relative_records(H.top, origin, rel);
    const size_t base = score(rel, axis);
    size_t best = base;
    for (int k = 0; k < 3; k++)
        for (float s : {2.0f, 4.0f}) {
            float ax[3] = {1.0f, 1.0f, 1.0f};
            ax[k] = s;
            if (!scaled_top_records(H, ax, origin, rel)) continue;
            double max_c2 = 0.0;
            std::vector<double> r2s;
            for (const auto& r : rel) {
                if (!std::isfinite(r.neg_r2)) continue;
                max_c2 = std::max(max_c2, (double)r.cx * r.cx + (double)r.cy * r.cy + (double)r.cz * r.cz);
                r2s.push_back(-(double)r.neg_r2);
            }
            if (r2s.empty()) continue;
            std::nth_element(r2s.begin(), r2s.begin() + r2s.size() / 2, r2s.end());
            if (!(kMfmaSlack * 2.0 * max_c2 <= 0.1 * r2s[r2s.size() / 2])) continue;
            const size_t met = score(rel, ax);
            if (met < best) { best = met; for (int q = 0; q < 3; q++) axis[q] = ax[q]; }
        }
    if (!((double)best <= 0.95 * (double)base)) axis[0] = axis[1] = axis[2] = 1.0f;
}

// the sweep's A operand, origin and D for a scene (`force`: a caller's D instead of the choice; diagnostics): the world-space top
// records for D = I (build_top_mfma, bit for bit), the records of scaled_top_records otherwise
void build_sweep_operand(const Hierarchy& H, const float* force, float axis[3], std::vector<uint16_t>& out, float origin[3],
                         double* max_c2, double* med_r2, size_t* n_real, std::vector<mrt::SphereRec>* rel_out) {
    sweep_origin(H.top, origin);
    if (force) for (int k = 0; k < 3; k++) axis[k] = force[k];
    else choose_sweep_axes(H, origin, axis);
    std::vector<mrt::SphereRec> rel;
    if (axis[0] == 1.0f && axis[1] == 1.0f && axis[2] == 1.0f) relative_records(H.top, origin, rel);
    else (void)scaled_top_records(H, axis, origin, rel);
    pack_top_mfma(rel, out, max_c2, med_r2, n_real);
    if (rel_out) rel_out->swap(rel);
}

// KParams::mfma_scale / mfma_neg_k2_pair for rays and records within `all` of the sweep's origin (mrt_debug_mfma_scale)
void mfma_scales(double all, float scale[4], uint32_t* neg_k2_pair) {
    if (!(all > 1e-30)) all = 1.0;
    int e = 0;
    (void)std::frexp(5.01 * all, &e);                       // 5.01 all < 2^e
    const double K = std::ldexp(1.0, -(e + 1)), K2 = K * K;
    scale[0] = (float)((double)mrt::kBoundStretch * K);
    scale[1] = (float)(2.0 * K2);
    scale[2] = (float)(-(1.0 - kMfmaSlack) * K2);
    scale[3] = (float)(16.0 * all * all);
    const uint32_t nk2 = (uint32_t)bf16_rne((float)-K2);    // a power of two: exact
    *neg_k2_pair = nk2 | (nk2 << 16);
}

// max over ALL spheres of |D (centre - origin)| + |radius| max D: no hit point lies further from the origin in the sweep's space
double sweep_reach(const float* centers4, const float* radii, uint32_t n, const float origin[3], const float axis[3]) {
    const double dmax = std::max(axis[0], std::max(axis[1], axis[2]));
    double reach = 0.0;
    for (uint32_t i = 0; i < n; i++) {
        double d2 = 0.0;
        for (int k = 0; k < 3; k++) { const double d = (double)axis[k] * ((double)centers4[4 * i + k] - (double)origin[k]); d2 += d * d; }
        reach = std::max(reach, std::sqrt(d2) + std::fabs((double)radii[i]) * dmax);
    }
    return reach;
}


}  // namespace mrt

using mrt::Hierarchy, mrt::build_hierarchy, mrt::build_top_mfma, mrt::build_sweep_operand, mrt::boxes_top_down, mrt::pack_boxes, mrt::mfma_scales;

namespace {
// what every mrt_debug_build_* entry point starts from: the caller's spheres as the builder takes them, and their hierarchy
struct BuiltScene {
    std::vector<float> centers, radii;
    Hierarchy h;
    BuiltScene(const mrt_sphere* spheres, size_t n, uint32_t max_levels, uint32_t top_target) : centers(4 * (n ? n : 1)), radii(n ? n : 1) {
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 3; k++) centers[4 * i + k] = spheres[i].center[k];
            centers[4 * i + 3] = 1.0f;
            radii[i] = spheres[i].radius;
        }
        build_hierarchy(centers.data(), radii.data(), (uint32_t)n, 8.0f, max_levels, top_target, h);
    }
};
}  // namespace

extern "C" {

int mrt_debug_build_hierarchy(const mrt_sphere* spheres, size_t n, uint32_t max_levels, uint32_t top_target,
                              float* top_out, size_t top_cap, float* nodes_out, size_t nodes_cap,
                              uint32_t* member_index_out, size_t member_cap, uint16_t* mfma_out, size_t mfma_cap,
                              float mfma_origin_out[3], uint32_t info[10]) {
    if ((!spheres && n) || !info || max_levels < 1 || max_levels > mrt::kMaxLevels || n > mrt::kMaxSpheres)
        return MRT_ERR_INVALID_ARG;
    const BuiltScene b(spheres, n, max_levels, top_target);
    const Hierarchy& h = b.h;
    std::vector<uint16_t> mf;
    float origin[3];
    double max_c2, med_r2;
    size_t n_real;
    build_top_mfma(h.top, mf, origin, &max_c2, &med_r2, &n_real);
    info[0] = h.levels; info[1] = (uint32_t)h.top.size(); info[2] = (uint32_t)h.nodes.size(); info[3] = h.n_members;
    info[4] = h.n_direct; info[5] = h.direct_first;
    for (uint32_t k = 0; k < mrt::kMaxLevels; k++) info[6 + k] = h.level_base[k];
    if ((top_out && top_cap < h.top.size()) || (nodes_out && nodes_cap < h.nodes.size()) ||
        (member_index_out && member_cap < h.member_index.size()) || (mfma_out && mfma_cap < mf.size()))
        return MRT_ERR_TOO_SMALL;
    if (top_out) std::memcpy(top_out, h.top.data(), h.top.size() * sizeof(mrt::SphereRec));
    if (nodes_out) std::memcpy(nodes_out, h.nodes.data(), h.nodes.size() * sizeof(mrt::SphereRec));
    if (member_index_out) std::memcpy(member_index_out, h.member_index.data(), h.member_index.size() * sizeof(uint32_t));
    if (mfma_out) std::memcpy(mfma_out, mf.data(), mf.size() * sizeof(uint16_t));
    if (mfma_origin_out) for (int k = 0; k < 3; k++) mfma_origin_out[k] = origin[k];
    return MRT_OK;
}

int mrt_debug_build_sweep(const mrt_sphere* spheres, size_t n, const float* force_axis, float axis_out[3], float* records_out,
                          size_t records_cap, uint16_t* mfma_out, size_t mfma_cap, float origin_out[3], double* reach_out) {
    if ((!spheres && n) || !axis_out || n > mrt::kMaxSpheres) return MRT_ERR_INVALID_ARG;
    if (force_axis)
        for (int k = 0; k < 3; k++)
            if (force_axis[k] != 1.0f && force_axis[k] != 2.0f && force_axis[k] != 4.0f) return MRT_ERR_INVALID_ARG;
    const BuiltScene b(spheres, n, mrt::kMaxLevels, 0);
    const Hierarchy& h = b.h;
    std::vector<uint16_t> mf;
    std::vector<mrt::SphereRec> rel;
    float origin[3];
    double max_c2, med_r2;
    size_t n_real;
    build_sweep_operand(h, force_axis, axis_out, mf, origin, &max_c2, &med_r2, &n_real, &rel);
    if ((records_out && records_cap < rel.size()) || (mfma_out && mfma_cap < mf.size())) return MRT_ERR_TOO_SMALL;
    if (records_out) std::memcpy(records_out, rel.data(), rel.size() * sizeof(mrt::SphereRec));
    if (mfma_out) std::memcpy(mfma_out, mf.data(), mf.size() * sizeof(uint16_t));
    if (origin_out) for (int k = 0; k < 3; k++) origin_out[k] = origin[k];
    if (reach_out) *reach_out = mrt::sweep_reach(b.centers.data(), b.radii.data(), (uint32_t)n, origin, axis_out);
    return MRT_OK;
}

int mrt_debug_build_boxes_top_down(const mrt_sphere* spheres, size_t n, uint32_t max_levels, uint32_t top_target, int open,
                                   float* boxes_out, size_t boxes_cap, uint32_t info[5]) {
    if ((!spheres && n) || !info || max_levels < 1 || max_levels > mrt::kMaxLevels || n > mrt::kMaxSpheres)
        return MRT_ERR_INVALID_ARG;
    const BuiltScene b(spheres, n, max_levels, top_target);
    const Hierarchy& h = b.h;
    std::vector<mrt::BoxFull> full;
    std::vector<mrt::BoxRec> packed;
    uint32_t cf = 0, cpf = 0;
    boxes_top_down(h, open != 0, full, &cf, &cpf);
    pack_boxes(full, packed);
    // what the kernel reads, in the 8-float form of mrt_debug_build_boxes: centre, the extents WITH kpad folded in, the scene's kc, 0
    std::vector<mrt::BoxFull> dev(full.size());
    for (size_t i = 0; i < full.size(); i++)
        dev[i] = mrt::BoxFull{packed[i].cx, packed[i].cy, packed[i].cz, packed[i].ex, packed[i].ey, packed[i].ez, full[i].ex >= 0.0f ? h.box_kc : 0.0f, 0.0f};
    info[0] = h.levels; info[1] = (uint32_t)dev.size(); info[2] = (uint32_t)h.top.size(); info[3] = cf; info[4] = cpf;
    if (boxes_out && boxes_cap < dev.size()) return MRT_ERR_TOO_SMALL;
    if (boxes_out) std::memcpy(boxes_out, dev.data(), dev.size() * sizeof(mrt::BoxFull));
    return MRT_OK;
}

int mrt_debug_build_boxes(const mrt_sphere* spheres, size_t n, uint32_t max_levels, uint32_t top_target, float* boxes_out,
                          size_t boxes_cap, uint32_t info[8]) {
    if ((!spheres && n) || !info || max_levels < 1 || max_levels > mrt::kMaxLevels || n > mrt::kMaxSpheres)
        return MRT_ERR_INVALID_ARG;
    const BuiltScene b(spheres, n, max_levels, top_target);
    const Hierarchy& h = b.h;
    info[0] = h.levels; info[1] = (uint32_t)h.boxes.size(); info[2] = h.box_quad ? 1u : 0u;
    for (uint32_t k = 0; k <= mrt::kMaxLevels; k++) info[3 + k] = h.box_base[k];
    if (boxes_out && boxes_cap < h.boxes.size()) return MRT_ERR_TOO_SMALL;
    if (boxes_out) std::memcpy(boxes_out, h.boxes.data(), h.boxes.size() * sizeof(mrt::BoxFull));
    return MRT_OK;
}

int mrt_debug_pool_clusters(const mrt_sphere* spheres, size_t n, uint32_t max_levels, uint32_t top_target, uint32_t* n_pool) {
    if ((!spheres && n) || !n_pool || max_levels < 1 || max_levels > mrt::kMaxLevels || n > mrt::kMaxSpheres) return MRT_ERR_INVALID_ARG;
    const BuiltScene b(spheres, n, max_levels, top_target);
    const Hierarchy& h = b.h;
    *n_pool = h.n_pool;
    return MRT_OK;
}

int mrt_debug_mfma_scale(double reach, float scale_out[4], uint32_t* neg_k2_bf16_pair_out) {
    if (!scale_out || !neg_k2_bf16_pair_out || !(reach >= 0.0) || !std::isfinite(reach)) return MRT_ERR_INVALID_ARG;
    mfma_scales(reach, scale_out, neg_k2_bf16_pair_out);
    return MRT_OK;
}

}  // extern "C"
