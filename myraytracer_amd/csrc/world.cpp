// The scene: mrt_set_world_raw / mrt_set_world (validation, the hierarchy of hierarchy.cpp, the uploads), the scene's part of
// the kernel arguments, and the scene-related diagnostics.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "mrt_ctx.h"
#include "hierarchy.h"

using mrt::fail, mrt::free_world, mrt::Hierarchy, mrt::build_hierarchy, mrt::build_sweep_operand, mrt::boxes_top_down, mrt::pack_boxes, mrt::kMfmaSlack, mrt::fill_scene_params;

namespace {

bool finite_in_range(float v, float lim) { return std::isfinite(v) && std::fabs(v) <= lim; }

// matrix-core sweep or SGPR-fed VALU sweep for the next launch: forced by mrt_debug_set_sweep,
// else the scene's verdict (mrt_set_world_raw) and the same test on the camera's distance from the origin
bool use_matrix_core_sweep(const mrt_ctx* c) {
    if (c->sweep_mode == 2) return true;
    if (c->sweep_mode == 1 || !c->mfma_scene_ok) return false;
    double o2 = 0.0;                              // squared distance of the camera from the GEMMs' origin, in the sweep's space
    for (int k = 0; k < 3; k++) {
        const double d = (double)c->mfma_axis[k] * ((c->cam_raw.mode ? (double)c->cam_raw.origin[k] : 0.0) - (double)c->mfma_origin[k]);
        o2 += d * d;
    }
    return kMfmaSlack * o2 <= 0.1 * c->mfma_r2_ref;
}

// launch_refit's arguments for the scene as the context holds it (mrt_update_spheres, mrt_regroup_spheres)
mrt::RefitArgs refit_args(const mrt_ctx* c) {
    const bool boxed = !mrt::scene_is_small(c->n_members);
    mrt::RefitArgs a;
    std::memset(&a, 0, sizeof a);
    a.spheres = c->d_spheres; a.shade = c->d_shade; a.member_index = c->d_member_index;
    a.nodes = c->d_nodes; a.clusters = c->d_clusters;
    a.boxes = boxed ? c->d_boxes : nullptr; a.boxes_open = boxed ? c->d_boxes_open : nullptr;
    a.top_mfma = c->d_top_mfma;
    a.n_members = c->n_members; a.n_hier = c->direct_first; a.levels = c->levels; a.n_nodes = c->n_nodes; a.n_padded = c->n_padded;
    for (uint32_t k = 0; k < mrt::kMaxLevels; k++) a.level_base[k] = c->level_base[k];
    a.box_quad = c->box_quad ? 1u : 0u; a.box_kc = c->box_kc;
    for (int k = 0; k < 3; k++) a.origin[k] = c->mfma_origin[k];
    return a;
}

// The auto-regroup policy (mrt_set_auto_regroup; regroup_policy.hip): its state is the tail of the regroup scratch, there for every
// scene with a pool of more than one cluster.  The judgement reads the records of the levels as the last refit left them.
mrt::RegroupState* regroup_state(const mrt_ctx* c) {
    return reinterpret_cast<mrt::RegroupState*>(c->d_regroup + mrt::regroup_layout(c->n_pool, c->n_pooled).state);
}
mrt::QualityArgs quality_args(const mrt_ctx* c, uint32_t mode, bool mark) {
    mrt::QualityArgs q;
    std::memset(&q, 0, sizeof q);
    q.nodes = c->d_nodes; q.clusters = c->d_clusters; q.state = regroup_state(c);
    q.levels = c->levels; q.n_nodes = c->n_nodes; q.n_padded = c->n_padded; q.n_pool = c->n_pool;
    for (uint32_t k = 0; k < mrt::kMaxLevels; k++) q.level_base[k] = c->level_base[k];
    q.mode = mode; q.mark = mark ? 1u : 0u; q.ratio = c->auto_regroup.ratio;
    return q;
}
mrt::RegroupArgs regroup_args(mrt_ctx* c, bool gated) {
    mrt::RegroupArgs g;
    g.spheres = c->d_spheres; g.member_index = c->d_member_index; g.scratch = c->d_regroup;
    g.n_pool = c->n_pool; g.pooled = c->n_pooled; g.block = c->regroup_block ? c->regroup_block : mrt::kRegroupBlock;
    g.gate = gated ? &regroup_state(c)->gate : nullptr;
    if (!gated) mrt::regroup_plan(g.n_pool, g.block, c->regroup_last);       // (whether a gated one ran, only the device knows)
    return g;
}

// The ordering of every call that changes device arrays of the scene behind the frames in flight (mrt_update_spheres,
// mrt_regroup_spheres, mrt_update_materials; `who` for the messages): the ctx's stream waits for the render kernels in flight,
// which read them; later frames wait for ev_inputs (inputs_dirty), recorded on the ctx's stream behind whatever the caller queues
// next (frames.cpp, enter_slot).  Nothing waits on the host.  -> MRT_OK, or MRT_ERR_HIP with the scene lost.
int lose_scene(mrt_ctx* c, const char* who, const char* what, hipError_t e) {
    c->have_world = false;
    return fail(c, MRT_ERR_HIP, "%s: %s failed: %s", who, what, hipGetErrorString(e));
}
int order_behind_frames(mrt_ctx* c, const char* who) {
    for (uint32_t i = 0; i < mrt_ctx::kMaxFrameSlots; i++) {
        mrt_ctx::FrameSlot& S = c->slot[i];
        if (!S.render_pending) continue;
        const hipError_t e = hipStreamWaitEvent(c->stream, S.render_done, 0);
        if (e != hipSuccess) return lose_scene(c, who, "hipStreamWaitEvent", e);
    }
    c->inputs_dirty = true;
    return MRT_OK;
}

// The geometry or the grouping changes (mrt_update_spheres, mrt_regroup_spheres): ordered as above; the camera masks, which are
// per cluster slot, are built anew; `change` queues what the call is about (-> 0 or a HIP error) and refit.hip derives
// everything else behind it, in stream order.  The refit's operand is the one for D = I: the scaled
// sweep space's proof (hierarchy.cpp, scaled_top_records) needs scene statistics only the device now has, so D = I until the next
// mrt_set_world*.  mfma_scene_ok / mfma_r2_ref stay the build's: they say where the matrix-core sweep's slack is small against
// R^2, a speed rule -- the sweep is conservative wherever it runs.  A failure leaves the device arrays between
// two scenes: the context then has no scene until the next mrt_set_world*.
// `rebaseline` (the auto-regroup policy, below): behind the refit, the policy's reference figure is taken anew where its state
// says "pending" -- the judgement queued by `change` opened the gate -- or, with kMark, in any case (a regroup the caller asked for).
enum Rebaseline { kNone, kIfPending, kMark };
template <class F> int change_scene(mrt_ctx* c, const char* who, F&& change, Rebaseline rebaseline = kNone) {
    auto lost = [&](const char* what, hipError_t e) { return lose_scene(c, who, what, e); };
    MRT_TRY(order_behind_frames(c, who));
    c->cam_mask_gen++;
    int le = change();
    if (le) return lost("launch", (hipError_t)le);
    c->mfma_axis[0] = c->mfma_axis[1] = c->mfma_axis[2] = 1.0f;
    le = mrt::launch_refit(refit_args(c), c->stream);
    if (le) return lost("launch", (hipError_t)le);
    if (rebaseline != kNone) {
        le = mrt::launch_regroup_quality(quality_args(c, mrt::kQualityBaseline, rebaseline == kMark), c->stream);
        if (le) return lost("launch", (hipError_t)le);
    }
    return MRT_OK;
}

bool auto_regroup_ok(const mrt_auto_regroup* p) {
    if (p->size != sizeof(mrt_auto_regroup) || p->enabled > 1 || p->check_every < 1 || p->check_every > 1024) return false;
    if (!(std::isfinite(p->ratio) && p->ratio >= 1.0f)) return false;
    for (uint32_t r : p->reserved)
        if (r != 0) return false;
    return true;
}

}  // namespace

namespace mrt {

// What shading a hit reads of a sphere's material (mrt_internal.h): the build's per-sphere derivation and mrt_update_materials'.
void material_shade(int32_t ty, const float* albedo, float param, float out[4]) {
    out[0] = out[1] = out[2] = 1.0f; out[3] = 0.0f;         // an unknown type absorbs: the kernel reads none of these
    if (ty == MRT_LAMBERTIAN) {
        std::memcpy(out, albedo, 3 * sizeof(float));
    } else if (ty == MRT_METAL) {
        std::memcpy(out, albedo, 3 * sizeof(float));
        out[3] = param;
    } else if (ty == MRT_DIELECTRIC) {
        // A Dielectric attenuates by (1,1,1) (a constant in the kernel), so its colour slots carry what its
        // scatter derives from the sphere alone, evaluated here with the same f32 operations in the same order
        // (correctly rounded '/', no contraction): ri = 1/ior for a front-face hit, and the Schlick r0 =
        // ((1-ri)/(1+ri))^2 for either face.  Bit-identical to evaluating them per hit.
        const float ior = param;
        auto schlick_r0 = [](float ri) { float r0 = (1.0f - ri) / (1.0f + ri); return r0 * r0; };
        const float inv_ior = 1.0f / ior;
        out[0] = inv_ior; out[1] = schlick_r0(inv_ior); out[2] = schlick_r0(ior);
        out[3] = ior;
    }
}

// the scene / hierarchy / sweep-variant part of the kernel arguments (everything that does not depend on the frame)
void fill_scene_params(const mrt_ctx* c, mrt::KParams& p) {
    p.world = c->world;
    p.cam = c->cam_raw;
    p.n_spheres = c->n_spheres;
    p.n_padded = c->n_padded;
    { const uint32_t ch = (c->n_padded + mrt::kChunk - 1) / mrt::kChunk; p.mask_chunks = ch < 16u ? ch : 16u; }
    {
        p.use_mfma = use_matrix_core_sweep(c) ? 1u : 0u;
        for (int k = 0; k < 3; k++) p.mfma_origin[k] = c->mfma_origin[k];
        // The sweep squares K oc.ds through an instruction that saturates at 1 (sweep.h, mfma_sweep_tile), K a power of
        // two: rays start on the camera's lens or on a sphere, i.e. within `all` of mfma_origin; the sweep admits origins up
        // to 4 x that (others take the literal loop), records lie within `all`, |ds| < 1.001: |K oc.ds| < 5.01 all K <= 1/2.
        // All of it in the sweep's space, x' = mfma_axis (x - mfma_origin): that is where the GEMMs run.
        double cam_d2 = 0.0, lens = 0.0;
        for (int k = 0; k < 3; k++) {
            p.mfma_axis[k] = c->mfma_axis[k];
            const double d = (double)c->mfma_axis[k] * ((c->cam_raw.mode ? (double)c->cam_raw.origin[k] : 0.0) - (double)c->mfma_origin[k]);
            cam_d2 += d * d;
        }
        p.mfma_scaled = (c->mfma_axis[0] != 1.0f || c->mfma_axis[1] != 1.0f || c->mfma_axis[2] != 1.0f) ? 1u : 0u;
        if (c->cam_raw.mode) {
            double u2 = 0.0, v2 = 0.0;
            for (int k = 0; k < 3; k++) {
                const double u = (double)c->mfma_axis[k] * c->cam_raw.ru[k], v = (double)c->mfma_axis[k] * c->cam_raw.rv[k];
                u2 += u * u; v2 += v * v;
            }
            lens = std::sqrt(u2) + std::sqrt(v2);
        }
        mfma_scales(std::max(c->mfma_reach, std::sqrt(cam_d2) + lens), p.mfma_scale, &p.mfma_neg_k2_pair);
    }
    p.levels = c->levels; p.n_nodes = c->n_nodes; p.n_members = c->n_members;
    // small scenes: the top queue holds a ray's candidates among ALL top records; large scenes: the wave's one work stack
    p.box_lds_count = mrt::scene_is_small(c->n_members) ? 0u : mrt::large_scene_box_lds_count(c->n_padded, c->levels, p.mask_chunks, mrt::kBoxLdsCap);
    p.gen_cap = mrt::scene_is_small(c->n_members) ? mrt::kSmallGenCap : mrt::large_scene_stack_cap(p.mask_chunks, p.box_lds_count);
    for (uint32_t k = 0; k < mrt::kMaxLevels; k++) p.level_base[k] = c->level_base[k];
    // large scenes only (kernels.hip: !SMALL): every node's box, in the kernel's top-down numbering
    p.boxes = c->boxes_mode == 0 ? c->d_boxes_open : c->d_boxes;
    p.box_cluster_first = c->box_cluster_first; p.box_cluster_parent_first = c->box_cluster_parent_first;
    p.box_quad = c->box_quad ? 1u : 0u;
    p.box_kc = c->box_kc;
    p.n_direct = c->n_direct; p.direct_first = c->direct_first;
    for (uint32_t k = 0; k < mrt::kMaxDirect; k++) { p.direct[k] = c->direct[k]; p.direct_index[k] = c->direct_index[k]; }
    p.cus = c->cus;
    p.spheres = c->d_spheres; p.clusters = c->d_clusters; p.nodes = c->d_nodes; p.top_mfma = c->d_top_mfma; p.member_index = c->d_member_index; p.vec4_data = c->d_vec4; p.shade = c->d_shade; p.f32_data = c->d_f32; p.i32_data = c->d_i32;
}

}  // namespace mrt

extern "C" {

int mrt_set_world_raw(mrt_ctx* c, const void* world, size_t world_bytes, const float* vec4, size_t n_vec4,
                      const float* f32, size_t n_f32, const int32_t* i32, size_t n_i32) {
    if (!c || !world) return MRT_ERR_INVALID_ARG;
    const auto t_begin = std::chrono::steady_clock::now();
    // 64 bytes = the reference's raw::World (lib.rs:676-684) as it is; 80 = with the DielectricRange extension.
    // Only world_bytes bytes of the caller's struct are read; a 64-byte World has no dielectrics.
    if (world_bytes != MRT_WORLD_BYTES_REFERENCE && world_bytes != sizeof(mrt_world))
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_set_world_raw: world_bytes %zu is neither %d (raw::World) nor %zu (mrt_world)",
                    world_bytes, MRT_WORLD_BYTES_REFERENCE, sizeof(mrt_world));
    mrt_world w_copy;
    std::memset(&w_copy, 0, sizeof w_copy);
    std::memcpy(&w_copy, world, world_bytes);
    const mrt_world* const w = &w_copy;
    if ((n_vec4 && !vec4) || (n_f32 && !f32) || (n_i32 && !i32)) return fail(c, MRT_ERR_INVALID_ARG, "mrt_set_world_raw: null array");
    const int64_t n = w->spheres.length;
    if (n < 0 || n > (int64_t)mrt::kMaxSpheres) return fail(c, MRT_ERR_BAD_SCENE, "spheres.length %lld out of range [0, %u]", (long long)n, mrt::kMaxSpheres);
    auto in_range = [](int64_t base, int64_t len, size_t cap) { return base >= 0 && len >= 0 && (uint64_t)(base + len) <= cap; };
    if (!in_range(w->spheres.center_base_idx, n, n_vec4) || !in_range(w->spheres.radius_base_idx, n, n_f32) ||
        !in_range(w->spheres.material_ty_base_idx, n, n_i32) || !in_range(w->spheres.material_idx_base_idx, n, n_i32) ||
        !in_range(w->lambertians.albedo_base_idx, w->lambertians.length, n_vec4) ||
        !in_range(w->metals.albedo_base_idx, w->metals.length, n_vec4) ||
        !in_range(w->metals.fuzz_base_idx, w->metals.length, n_f32) ||
        !in_range(w->dielectrics.ior_base_idx, w->dielectrics.length, n_f32))
        return fail(c, MRT_ERR_BAD_SCENE, "a World range points outside its data array");
    // geometry must be finite and moderate so that no discriminant can overflow to inf/NaN
    const float kLim = 1.0e7f;
    for (int64_t i = 0; i < n; i++) {
        const float* ctr = vec4 + 4 * (w->spheres.center_base_idx + i);
        const float r = f32[w->spheres.radius_base_idx + i];
        if (!finite_in_range(ctr[0], kLim) || !finite_in_range(ctr[1], kLim) || !finite_in_range(ctr[2], kLim) ||
            !finite_in_range(r, kLim))
            return fail(c, MRT_ERR_BAD_SCENE, "sphere %lld: centre/radius not finite or |v| > 1e7", (long long)i);
        const int32_t ty = i32[w->spheres.material_ty_base_idx + i];
        const int32_t mi = i32[w->spheres.material_idx_base_idx + i];
        const int32_t len = ty == MRT_LAMBERTIAN ? w->lambertians.length : ty == MRT_METAL ? w->metals.length
                          : ty == MRT_DIELECTRIC ? w->dielectrics.length : INT32_MAX;   // unknown ty: absorbs, idx unused
        if (mi < 0 || (ty >= MRT_LAMBERTIAN && ty <= MRT_DIELECTRIC && mi >= len))
            return fail(c, MRT_ERR_BAD_SCENE, "sphere %lld: material index %d out of range for type %d", (long long)i, mi, ty);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    free_world(c);

    // exact-test records, in the reference's sphere order
    std::vector<mrt::SphereRec> recs((size_t)n ? (size_t)n : 1);
    for (int64_t i = 0; i < n; i++) {
        const float* ctr = vec4 + 4 * (w->spheres.center_base_idx + i);
        const float r = f32[w->spheres.radius_base_idx + i];
        recs[(size_t)i] = mrt::SphereRec{ctr[0], ctr[1], ctr[2], -(r * r)};
    }
    // bounding-sphere hierarchy over spatially close spheres; the sweep tests its top level
    Hierarchy hier;
    build_hierarchy(vec4 + 4 * w->spheres.center_base_idx, f32 + w->spheres.radius_base_idx, (uint32_t)n,
                    c->cluster_factor, c->max_levels, c->top_target, hier);
    const uint32_t n_padded = (uint32_t)hier.top.size();
    auto upload = [&](void** dst, const void* src, size_t bytes) -> int {
        HIP_TRY(c, hipMalloc(dst, bytes ? bytes : 16));
        if (bytes) HIP_TRY(c, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return MRT_OK;
    };
    MRT_TRY(upload((void**)&c->d_spheres, recs.data(), recs.size() * sizeof(mrt::SphereRec)));
    MRT_TRY(upload((void**)&c->d_clusters, hier.top.data(), hier.top.size() * sizeof(mrt::SphereRec)));
    MRT_TRY(upload((void**)&c->d_nodes, hier.nodes.data(), hier.nodes.size() * sizeof(mrt::SphereRec)));
    if (!mrt::scene_is_small(hier.n_members)) {           // large scenes (the kernel's !SMALL layouts) walk the boxes
        std::vector<mrt::BoxFull> full;
        std::vector<mrt::BoxRec> dev;
        boxes_top_down(hier, false, full, &c->box_cluster_first, &c->box_cluster_parent_first);
        pack_boxes(full, dev);
        MRT_TRY(upload((void**)&c->d_boxes, dev.data(), dev.size() * sizeof(mrt::BoxRec)));
        boxes_top_down(hier, true, full, &c->box_cluster_first, &c->box_cluster_parent_first);
        pack_boxes(full, dev);
        MRT_TRY(upload((void**)&c->d_boxes_open, dev.data(), dev.size() * sizeof(mrt::BoxRec)));
    }
    c->box_quad = hier.box_quad;
    c->box_kc = hier.box_kc;
    {
        std::vector<uint16_t> top_mfma;
        double max_c2 = 0.0, med_r2 = 0.0;
        size_t n_real = 0;
        build_sweep_operand(hier, c->have_force_axis ? c->force_axis : nullptr, c->mfma_axis, top_mfma, c->mfma_origin, &max_c2,
                            &med_r2, &n_real, nullptr);
        MRT_TRY(upload((void**)&c->d_top_mfma, top_mfma.data(), top_mfma.size() * sizeof(uint16_t)));
        // The matrix-core sweep inflates R^2 by 2^-13 (o.o + C.C + R^2), o and C relative to mfma_origin in the sweep's
        // space (x' = mfma_axis (x - mfma_origin)); rays start in or around the scene.
        // Selected where that stays below about a tenth of the typical R^2 (mrt_redraw checks the camera's
        // own distance the same way) and there are enough records to fill most of a 32-record tile.
        c->mfma_r2_ref = med_r2;
        c->mfma_reach = mrt::sweep_reach(vec4 + 4 * w->spheres.center_base_idx, f32 + w->spheres.radius_base_idx, (uint32_t)n,
                                         c->mfma_origin, c->mfma_axis);
        c->mfma_scene_ok = n_real >= 24 && med_r2 > 0.0 && kMfmaSlack * 2.0 * max_c2 <= 0.1 * med_r2;
    }
    MRT_TRY(upload((void**)&c->d_member_index, hier.member_index.data(), hier.member_index.size() * sizeof(uint32_t)));
    if (mrt::scene_is_small(hier.n_members) && n_padded <= mrt::kCamMaskRecords) {
        // the camera-ray cluster masks (cam_mask.hip; frames.cpp builds them before a frame when it pays): an entry of 4 words per
        // 8 texels of the shard as it is now, all ones until built.  A shard that outgrows it renders without masks.  Behind
        // them, in the same buffer, the camera-ray sphere lists of the same entries (mrt_ctx::cam_lists), 4 words each: all
        // ones is "overflowed" there.
        const size_t entries = std::max<size_t>((mrt::local_texels(c) + 7) / 8, 1);
        const std::vector<uint32_t> ones(8 * entries, 0xFFFFFFFFu);
        MRT_TRY(upload((void**)&c->d_cam_masks, ones.data(), ones.size() * sizeof(uint32_t)));
        c->cam_mask_entries = entries;
    }
    {
        // The regroup scratch (mrt_regroup_spheres; mrt_internal.h, regroup_layout): what a regroup reads of the build -- the pool's
        // sphere indices ascending, the cluster of every rank, pref -- and the room it works in: 16 bytes a pooled sphere for the
        // lists and orders, 7 a cluster for pref and the boxes, 8 a key of the sort (a power of two of at least 2,048, below twice
        // the pool): under 64 bytes a pooled sphere beyond the smallest scenes.  A scene without a pool gets the 16-byte stub.
        uint32_t pooled = 0;
        std::vector<uint32_t> pref((size_t)hier.n_pool + 1, 0u);
        for (uint32_t k = 0; k < hier.n_pool; k++) {
            for (uint32_t m = 0; m < mrt::kClusterK; m++) pooled += std::isfinite(hier.nodes[(size_t)mrt::kClusterK * k + m].neg_r2) ? 1u : 0u;
            pref[k + 1] = pooled;
        }
        std::vector<uint32_t> scratch;
        if (hier.n_pool > 1) {
            const mrt::RegroupLayout L = mrt::regroup_layout(hier.n_pool, pooled);
            scratch.assign(L.words, 0u);
            for (uint32_t k = 0, at = 0; k < hier.n_pool; k++)
                for (uint32_t m = 0; m < mrt::kClusterK; m++)
                    if (std::isfinite(hier.nodes[(size_t)mrt::kClusterK * k + m].neg_r2)) {
                        scratch[L.pool + at] = hier.member_index[(size_t)mrt::kClusterK * k + m];
                        scratch[L.clus + at] = k;
                        at++;
                    }
            std::sort(scratch.begin() + (long)L.pool, scratch.begin() + (long)(L.pool + pooled));
            std::copy(pref.begin(), pref.end(), scratch.begin() + (long)L.pref);
            // the auto-regroup policy's state: baseline pending, counters 0 (the device's alone from here on)
            mrt::RegroupState st0;
            std::memset(&st0, 0, sizeof st0);
            st0.pending = 1u;
            std::memcpy(scratch.data() + L.state, &st0, sizeof st0);
        }
        MRT_TRY(upload((void**)&c->d_regroup, scratch.data(), scratch.size() * sizeof(uint32_t)));
        c->n_pool = hier.n_pool; c->n_pooled = pooled;
        c->regroup_words = scratch.size();
        c->auto_updates = 0;
        c->regroup_last[0] = c->regroup_last[1] = c->regroup_last[2] = 0;
    }
    // what shading a hit on sphere i reads, gathered per sphere (bit copies of the SoA entries)
    std::vector<float> shade(8 * ((size_t)n ? (size_t)n : 1), 0.0f);
    for (int64_t i = 0; i < n; i++) {
        const float* ctr = vec4 + 4 * (w->spheres.center_base_idx + i);
        float* sh = shade.data() + 8 * (size_t)i;
        sh[0] = ctr[0]; sh[1] = ctr[1]; sh[2] = ctr[2];
        sh[3] = f32[w->spheres.radius_base_idx + i];
        const int32_t ty = i32[w->spheres.material_ty_base_idx + i];
        const int32_t mi = i32[w->spheres.material_idx_base_idx + i];
        // (an unknown type's index is unused; material_shade is mrt_update_materials' derivation too)
        const float* albedo = ty == MRT_LAMBERTIAN ? vec4 + 4 * (w->lambertians.albedo_base_idx + mi)
                            : ty == MRT_METAL ? vec4 + 4 * (w->metals.albedo_base_idx + mi) : nullptr;
        const float param = ty == MRT_METAL ? f32[w->metals.fuzz_base_idx + mi] : ty == MRT_DIELECTRIC ? f32[w->dielectrics.ior_base_idx + mi] : 0.0f;
        mrt::material_shade(ty, albedo, param, sh + 4);
    }
    MRT_TRY(upload((void**)&c->d_shade, shade.data(), shade.size() * sizeof(float)));
    {
        // temporal reprojection's "previous" spheres (mrt_temporal_step snapshots into it): (cx, cy, cz, r) each, the scene's own to begin with
        std::vector<float> xyzr(4 * ((size_t)n ? (size_t)n : 1), 0.0f);
        for (int64_t i = 0; i < n; i++) std::memcpy(xyzr.data() + 4 * (size_t)i, shade.data() + 8 * (size_t)i, 4 * sizeof(float));
        MRT_TRY(upload((void**)&c->d_prev_xyzr, xyzr.data(), xyzr.size() * sizeof(float)));
    }
    MRT_TRY(upload((void**)&c->d_vec4, vec4, n_vec4 * 4 * sizeof(float)));
    MRT_TRY(upload((void**)&c->d_f32, f32, n_f32 * sizeof(float)));
    MRT_TRY(upload((void**)&c->d_i32, i32, n_i32 * sizeof(int32_t)));
    for (auto& S : c->slot) S.cost_valid = false;
    c->width.invalidate();              // (the launch-width controller starts over with the new workload)
    c->inputs_dirty = true;
    c->world = *w;
    c->n_spheres = (uint32_t)n;
    c->n_padded = n_padded;
    c->levels = hier.levels; c->n_nodes = (uint32_t)hier.nodes.size(); c->n_members = hier.n_members;
    for (uint32_t k = 0; k < mrt::kMaxLevels; k++) c->level_base[k] = hier.level_base[k];
    c->n_direct = hier.n_direct; c->direct_first = hier.direct_first;
    for (uint32_t k = 0; k < mrt::kMaxDirect; k++) { c->direct[k] = hier.direct[k]; c->direct_index[k] = hier.direct_index[k]; }
    c->have_world = true;
    c->set_world_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return MRT_OK;
}

int mrt_debug_last_set_world_ms(mrt_ctx* c, float* ms) {
    if (!c || !ms) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_debug_last_set_world_ms: no scene");
    *ms = c->set_world_ms;
    return MRT_OK;
}

int mrt_set_world(mrt_ctx* c, const mrt_sphere* spheres, size_t n) {
    if (!c || (!spheres && n)) return MRT_ERR_INVALID_ARG;
    std::vector<float> vec4(8 * n + 4), f32(2 * n + 1);
    std::vector<int32_t> i32(2 * n + 1);
    mrt_world w;
    size_t nv = 0, nf = 0, ni = 0;
    int st = mrt_pack_world(spheres, n, &w, vec4.data(), 2 * n + 1, &nv, f32.data(), 2 * n + 1, &nf, i32.data(), 2 * n + 1, &ni);
    if (st != MRT_OK) return fail(c, st, "mrt_set_world: packing failed (%s)", mrt_status_string(st));
    return mrt_set_world_raw(c, &w, sizeof w, vec4.data(), nv, f32.data(), nf, i32.data(), ni);
}

// New geometry for spheres whose grouping stays (include/myraytracer_amd.h): O(count) work here, everything derived from the
// spheres recomputed by refit.hip in stream order.  Nothing waits on the host: the ctx's stream is made to wait for the render
// kernels in flight (they read the arrays about to change), and every later frame's side stream waits for ev_inputs, recorded
// on the ctx's stream behind the refit (frames.cpp, enter_slot).  The updates travel in kernel arguments, kRefitBatch spheres a
// launch: a hipMemcpyAsync from the caller's pageable memory would have the runtime stage the data and order the copy itself --
// it may hold the calling thread until the stream has drained -- and needs a staging buffer of ours to be safe from the caller
// reusing xyzr; arguments are copied at the launch call and need neither.
int mrt_update_spheres(mrt_ctx* c, uint32_t first, uint32_t count, const float* xyzr) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_update_spheres: no scene");
    if ((uint64_t)first + count > c->n_spheres)
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_update_spheres: spheres [%u, %llu) of a scene of %u", first, (unsigned long long)first + count, c->n_spheres);
    if (count && !xyzr) return fail(c, MRT_ERR_INVALID_ARG, "mrt_update_spheres: null array");
    for (size_t i = 0; i < 4 * (size_t)count; i++)
        if (!finite_in_range(xyzr[i], 1.0e7f))
            return fail(c, MRT_ERR_BAD_SCENE, "mrt_update_spheres: sphere %zu: centre/radius not finite or |v| > 1e7", first + i / 4);
    if (count == 0) return MRT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // The auto-regroup policy: every check_every-th call queues, behind the scatter, the judgement of the hierarchy and the regroup
    // whose kernels the judgement's gate word lets run or return at once; the refit follows in any case, and the policy's
    // reference figure is taken anew behind it where the gate opened.  The judgement reads the bounds of the PREVIOUS update's
    // refit -- those the last frames were rendered with -- so no second, gated refit is needed.  The host never learns the verdict.
    const bool check = c->auto_regroup.enabled && c->n_pool > 1 && (c->auto_updates + 1) % c->auto_regroup.check_every == 0;
    const int st = change_scene(c, "mrt_update_spheres", [&]() -> int {
        c->guides_stale = true;
        const bool boxed = !mrt::scene_is_small(c->n_members);
        double reach = c->mfma_reach;
        float kc = c->box_kc;
        for (uint32_t b = 0; b < count; b += mrt::kRefitBatch) {
            mrt::RefitScatterArgs s;
            s.spheres = c->d_spheres; s.shade = c->d_shade;
            s.centres = c->d_vec4 + 4 * (size_t)c->world.spheres.center_base_idx;
            s.radii = c->d_f32 + c->world.spheres.radius_base_idx;
            s.first = first + b; s.count = std::min(mrt::kRefitBatch, count - b);
            std::memcpy(s.xyzr, xyzr + 4 * (size_t)b, 16 * (size_t)s.count);
            const int le = mrt::launch_refit_scatter(s, c->stream);
            if (le) return le;
            // The scene-level kernel arguments, kept valid monotonically from the updated spheres alone: the sweep's reach (D = I
            // from here on; a reach measured in a scaled space only overstates it), the direct spheres' records, and the box slack's
            // kc >= quad_kc_for_radius of every clustered sphere (the quadratic form; both forms are valid bounds, so the form stays).
            for (uint32_t i = 0; i < s.count; i++) {
                const float* v = s.xyzr + 4 * i;
                const uint32_t idx = s.first + i;
                double d2 = 0.0;
                for (int k = 0; k < 3; k++) { const double d = (double)v[k] - (double)c->mfma_origin[k]; d2 += d * d; }
                reach = std::max(reach, std::sqrt(d2) + std::fabs((double)v[3]));
                bool direct = false;
                for (uint32_t k = 0; k < c->n_direct; k++)
                    if (c->direct_index[k] == idx) { c->direct[k] = mrt::SphereRec{v[0], v[1], v[2], -(v[3] * v[3])}; direct = true; }
                if (boxed && c->box_quad && !direct) kc = std::max(kc, mrt::round_up_f32(mrt::quad_kc_for_radius(std::fabs((double)v[3]))));
            }
        }
        c->mfma_reach = reach;
        c->box_kc = kc;
        if (!check) return 0;
        const int le = mrt::launch_regroup_quality(quality_args(c, mrt::kQualityDecide, false), c->stream);
        return le ? le : mrt::launch_regroup(regroup_args(c, true), c->stream);
    }, check ? kIfPending : kNone);
    if (st == MRT_OK && c->auto_regroup.enabled && c->n_pool > 1) c->auto_updates++;
    return st;
}

// New materials for spheres whose geometry stays (include/myraytracer_amd.h): the two things shading reads of a sphere's material
// -- floats 4..7 of its shade record and its type word -- derived here by the build's own function and scattered in stream order,
// kMaterialBatch spheres a launch, in the kernel arguments as a geometry update's are.  Ordered like an update and nothing more:
// no refit (the hierarchy does not know materials), no new camera masks (geometry only), the sweep's space, the schedule, the
// tile costs and the auto-regroup policy's count as they are.  The SoA copies of the materials on the device (albedo / fuzz /
// ior entries, material_idx) are left as the last mrt_set_world* wrote them: no kernel reads them.
int mrt_update_materials(mrt_ctx* c, uint32_t first, uint32_t count, const mrt_material* materials, uint32_t flags) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)MRT_MATERIALS_RESTART_HISTORY) return fail(c, MRT_ERR_INVALID_ARG, "mrt_update_materials: flags 0x%x", flags);
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_update_materials: no scene");
    if ((uint64_t)first + count > c->n_spheres)
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_update_materials: spheres [%u, %llu) of a scene of %u", first, (unsigned long long)first + count, c->n_spheres);
    if (count && !materials) return fail(c, MRT_ERR_INVALID_ARG, "mrt_update_materials: null array");
    if (count == 0) return MRT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(order_behind_frames(c, "mrt_update_materials"));
    c->guides_stale = true;             // (the albedo guide, and its rule for a Dielectric)
    for (uint32_t b = 0; b < count; b += mrt::kMaterialBatch) {
        mrt::MaterialScatterArgs s;
        s.shade = c->d_shade; s.types = c->d_i32 + c->world.spheres.material_ty_base_idx; s.prev_xyzr = c->d_prev_xyzr;
        s.first = first + b; s.count = std::min(mrt::kMaterialBatch, count - b);
        s.restart_history = (flags & MRT_MATERIALS_RESTART_HISTORY) ? 1u : 0u; s._pad = 0;
        for (uint32_t i = 0; i < s.count; i++) {
            const mrt_material& m = materials[(size_t)b + i];
            mrt::material_shade(m.material_ty, m.albedo, m.param, s.words + 4 * i);
            s.ty[i] = m.material_ty;
        }
        const int le = mrt::launch_material_scatter(s, c->stream);
        if (le) return lose_scene(c, "mrt_update_materials", "launch", (hipError_t)le);
    }
    return MRT_OK;
}

int mrt_debug_material_shade(const mrt_material* material, float out[4]) {
    if (!material || !out) return MRT_ERR_INVALID_ARG;
    mrt::material_shade(material->material_ty, material->albedo, material->param, out);
    return MRT_OK;
}

// The grouping made anew from the spheres as the device holds them (include/myraytracer_amd.h): regroup.hip permutes the pooled
// spheres over their member slots, refit.hip derives everything from the new order.  Ordered like an update: the ctx's stream
// waits for the render kernels in flight, later frames wait for ev_inputs; nothing waits on the host.
int mrt_regroup_spheres(mrt_ctx* c) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_regroup_spheres: no scene");
    if (c->n_pool <= 1) return MRT_OK;                  // no clustering, or nothing to trade between clusters
    HIP_TRY(c, hipSetDevice(c->device));
    // (the guides stay current: the geometry did not change; with the auto-regroup policy on, its reference figure is this grouping's)
    return change_scene(c, "mrt_regroup_spheres", [&]() -> int { return mrt::launch_regroup(regroup_args(c, false), c->stream); },
                        c->auto_regroup.enabled ? kMark : kNone);
}

void mrt_auto_regroup_default(mrt_auto_regroup* out) {
    if (out) *out = mrt::auto_regroup_defaults();
}

int mrt_set_auto_regroup(mrt_ctx* c, const mrt_auto_regroup* p) {
    if (!p) return MRT_ERR_INVALID_ARG;
    if (!auto_regroup_ok(p))
        return !c ? (int)MRT_ERR_INVALID_ARG : fail(c, MRT_ERR_INVALID_ARG, "mrt_set_auto_regroup: size %u (%zu), enabled %u (0, 1), check_every %u (1..1024), "
                    "ratio %g (finite, >= 1), reserved 0", p->size, sizeof(mrt_auto_regroup), p->enabled, p->check_every, (double)p->ratio);
    if (!c) return MRT_OK;              // (ctx NULL: a check of the setting alone)
    // turned on with a scene present: the reference figure is the hierarchy's as it is now, taken in stream order
    if (p->enabled && !c->auto_regroup.enabled && c->have_world && c->n_pool > 1) {
        HIP_TRY(c, hipSetDevice(c->device));
        const int le = mrt::launch_regroup_quality(quality_args(c, mrt::kQualityBaseline, true), c->stream);
        if (le) { c->have_world = false; return fail(c, MRT_ERR_HIP, "mrt_set_auto_regroup: launch failed: %s", hipGetErrorString((hipError_t)le)); }
    }
    c->auto_regroup = *p;
    c->auto_updates = 0;
    return MRT_OK;
}

int mrt_get_auto_regroup(mrt_ctx* c, mrt_auto_regroup* out) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    *out = c->auto_regroup;
    return MRT_OK;
}

int mrt_read_regroup_stats(mrt_ctx* c, mrt_regroup_stats* out) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_read_regroup_stats: no scene");
    std::memset(out, 0, sizeof *out);
    if (c->n_pool <= 1) return MRT_OK;                  // no pool to regroup: the policy never checks
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_stream(c, c->stream, "mrt_read_regroup_stats"));
    mrt::RegroupState s;
    HIP_TRY(c, hipMemcpy(&s, regroup_state(c), sizeof s, hipMemcpyDeviceToHost));
    out->checks = s.checks; out->regroups = s.regroups; out->q_ref = s.q_ref; out->q_last = s.q_last;
    for (uint32_t k = 0; k < mrt::kMaxLevels; k++) out->q_level[k] = s.q_level[k];
    out->levels = c->levels; out->pending = s.pending;
    return MRT_OK;
}

int mrt_debug_regroup_info(mrt_ctx* c, uint32_t out[4]) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_debug_regroup_info: no scene");
    uint32_t plan[3];
    mrt::regroup_plan(c->n_pool, c->regroup_block ? c->regroup_block : mrt::kRegroupBlock, plan);
    out[0] = c->n_pool; out[1] = plan[0]; out[2] = c->regroup_last[1]; out[3] = c->regroup_last[2];
    return MRT_OK;
}

int mrt_debug_set_regroup_block(mrt_ctx* c, uint32_t clusters) {
    if (!c || (clusters != 0 && (clusters < 4 || clusters > mrt::kRegroupBlock || (clusters & (clusters - 1))))) return MRT_ERR_INVALID_ARG;
    c->regroup_block = clusters;
    return MRT_OK;
}

int mrt_debug_read_hierarchy(mrt_ctx* c, uint32_t info[16], double scalars[8], float* direct_out, uint32_t* direct_index_out,
                             float* top_out, float* nodes_out, uint32_t* member_index_out, float* boxes_out, float* boxes_open_out,
                             uint16_t* mfma_out, float* spheres_out, float* shade_out, float* centres_out, float* radii_out) {
    if (!c || !info) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_debug_read_hierarchy: no scene");
    const bool boxed = !mrt::scene_is_small(c->n_members);
    size_t n_boxes = 0;
    if (boxed) for (uint32_t t = 0; t < c->levels; t++) n_boxes += (size_t)c->n_padded << (2 * t);
    info[0] = c->levels; info[1] = c->n_padded; info[2] = c->n_nodes; info[3] = c->n_members; info[4] = c->n_direct; info[5] = c->direct_first;
    for (uint32_t k = 0; k < mrt::kMaxLevels; k++) info[6 + k] = c->level_base[k];
    info[10] = (uint32_t)n_boxes; info[11] = c->box_quad ? 1u : 0u; info[12] = c->n_spheres; info[13] = c->box_cluster_first;
    info[14] = c->box_cluster_parent_first; info[15] = c->mfma_scene_ok ? 1u : 0u;
    if (scalars) {
        scalars[0] = (double)c->box_kc;
        for (int k = 0; k < 3; k++) { scalars[1 + k] = (double)c->mfma_origin[k]; scalars[4 + k] = (double)c->mfma_axis[k]; }
        scalars[7] = c->mfma_reach;
    }
    if (direct_out) std::memcpy(direct_out, c->direct, sizeof c->direct);
    if (direct_index_out) std::memcpy(direct_index_out, c->direct_index, sizeof c->direct_index);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_stream(c, c->stream, "mrt_debug_read_hierarchy"));
    auto read = [&](void* dst, const void* src, size_t bytes) -> int {
        if (dst && bytes) HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return MRT_OK;
    };
    const size_t n = c->n_spheres;
    MRT_TRY(read(top_out, c->d_clusters, (size_t)c->n_padded * sizeof(mrt::SphereRec)));
    MRT_TRY(read(nodes_out, c->d_nodes, (size_t)c->n_nodes * sizeof(mrt::SphereRec)));
    MRT_TRY(read(member_index_out, c->d_member_index, (size_t)c->n_members * sizeof(uint32_t)));
    MRT_TRY(read(boxes_out, c->d_boxes, n_boxes * sizeof(mrt::BoxRec)));
    MRT_TRY(read(boxes_open_out, c->d_boxes_open, n_boxes * sizeof(mrt::BoxRec)));
    MRT_TRY(read(mfma_out, c->d_top_mfma, (size_t)c->n_padded / 32 * 512 * sizeof(uint16_t)));
    MRT_TRY(read(spheres_out, c->d_spheres, n * sizeof(mrt::SphereRec)));
    MRT_TRY(read(shade_out, c->d_shade, n * 8 * sizeof(float)));
    MRT_TRY(read(centres_out, c->d_vec4 + 4 * (size_t)c->world.spheres.center_base_idx, n * 4 * sizeof(float)));
    MRT_TRY(read(radii_out, c->d_f32 + c->world.spheres.radius_base_idx, n * sizeof(float)));
    return MRT_OK;
}

// diagnostic / tuning: cluster growth factor used by the NEXT mrt_set_world* call
int mrt_debug_set_cluster_factor(mrt_ctx* c, float factor) {
    if (!c || !(factor >= 0.0f)) return MRT_ERR_INVALID_ARG;
    c->cluster_factor = factor;
    return MRT_OK;
}

int mrt_debug_set_sweep_axes(mrt_ctx* c, const float* axis) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (axis)
        for (int k = 0; k < 3; k++)
            if (axis[k] != 1.0f && axis[k] != 2.0f && axis[k] != 4.0f) return MRT_ERR_INVALID_ARG;
    c->have_force_axis = axis != nullptr;
    for (int k = 0; k < 3; k++) c->force_axis[k] = axis ? axis[k] : 1.0f;
    return MRT_OK;
}

int mrt_debug_set_camera_masks(mrt_ctx* c, int on) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (on < 0 || on > 3) return MRT_ERR_INVALID_ARG;
    c->cam_masks_on = on != 0;
    c->cam_prefer = on >= 2 ? (uint32_t)on - 1u : 0u;
    return MRT_OK;
}

int mrt_debug_read_camera_masks(mrt_ctx* c, uint32_t info[4], uint32_t* out, size_t cap_words) {
    if (!c || !info) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_debug_read_camera_masks: no scene");
    const size_t need = (mrt::local_texels(c) + 7) / 8;
    const bool fits = c->d_cam_masks && need != 0 && need <= c->cam_mask_entries;
    info[0] = fits ? (uint32_t)need : 0u;
    info[1] = 4u;
    info[2] = c->cam_masks_in_force ? (c->cam_lists_in_force ? 2u : 1u) : 0u;
    info[3] = fits && c->cam_mask_built == c->cam_mask_gen ? 1u : 0u;
    if (!out || !fits) return MRT_OK;
    if (cap_words < 4 * need) return fail(c, MRT_ERR_TOO_SMALL, "mrt_debug_read_camera_masks: need %zu words", 4 * need);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, "mrt_debug_read_camera_masks"));             // (the build runs on a frame's side stream)
    HIP_TRY(c, hipMemcpy(out, c->d_cam_masks, 4 * need * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MRT_OK;
}

int mrt_debug_read_camera_lists(mrt_ctx* c, uint32_t info[4], uint32_t* out, size_t cap_words) {
    if (!c || !info) return MRT_ERR_INVALID_ARG;
    MRT_TRY(mrt_debug_read_camera_masks(c, info, nullptr, 0));
    const size_t need = info[0];
    if (!out || need == 0) return MRT_OK;
    if (cap_words < 4 * need) return fail(c, MRT_ERR_TOO_SMALL, "mrt_debug_read_camera_lists: need %zu words", 4 * need);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, "mrt_debug_read_camera_lists"));
    HIP_TRY(c, hipMemcpy(out, c->cam_lists(), 4 * need * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MRT_OK;
}

int mrt_debug_sweep_axes(mrt_ctx* c, float axis_out[3]) {
    if (!c || !axis_out) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_debug_sweep_axes: no scene");
    for (int k = 0; k < 3; k++) axis_out[k] = c->mfma_axis[k];
    return MRT_OK;
}

int mrt_debug_set_sweep(mrt_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2) return MRT_ERR_INVALID_ARG;
    c->sweep_mode = mode;
    return MRT_OK;
}

int mrt_debug_world_hit_stats(mrt_ctx* c, uint64_t out[2]) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    out[0] = c->dbg_world_hit_stats[0]; out[1] = c->dbg_world_hit_stats[1];
    return MRT_OK;
}

int mrt_debug_world_hit(mrt_ctx* c, const float* rays, size_t n, int32_t* hit_out, uint32_t* cand_out, size_t cand_words) {
    if (!c || !rays || !hit_out || n == 0) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_debug_world_hit: no scene");
    const size_t need_words = ((size_t)c->n_spheres + 31) / 32;
    if (cand_out && cand_words < need_words) return fail(c, MRT_ERR_TOO_SMALL, "mrt_debug_world_hit: need %zu bitmap words per ray", need_words);
    if (n > (1u << 26)) return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_world_hit: too many rays");
    for (size_t i = 0; i < 6 * n; i++)
        if (!(std::fabs(rays[i]) <= 2.0e7f)) return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_world_hit: ray %zu is not finite or beyond 2e7", i / 6);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    // rays become the texels of an 8-pixel-wide virtual image (one 8x8 tile per 64 rays), padded with copies of ray 0
    const size_t n_rays = (n + 63) / 64 * 64;
    // rows allocated: 64 spare rows of candidate words (>= 256 bytes) hold the launch's 16 counters, cleared and read back with them
    const size_t n_pad = n_rays + 64;
    const size_t words = need_words ? need_words : 1;
    std::vector<float> host_rays(6 * n_rays);
    std::memcpy(host_rays.data(), rays, 6 * n * sizeof(float));
    for (size_t i = n; i < n_rays; i++) std::memcpy(host_rays.data() + 6 * i, rays, 6 * sizeof(float));
    float* d_rays = nullptr; int32_t* d_hit = nullptr; uint32_t* d_cand = nullptr; uint32_t* d_queue = nullptr;
    auto cleanup = [&]() { (void)hipFree(d_rays); (void)hipFree(d_hit); (void)hipFree(d_cand); (void)hipFree(d_queue); };
    hipError_t e = hipSuccess;
    const char* what = "the upload";
    HIP_CHAIN(e, what, hipMalloc((void**)&d_rays, host_rays.size() * sizeof(float)));
    HIP_CHAIN(e, what, hipMalloc((void**)&d_hit, n_pad * 2 * sizeof(int32_t)));
    HIP_CHAIN(e, what, hipMalloc((void**)&d_cand, n_pad * words * sizeof(uint32_t)));
    HIP_CHAIN(e, what, hipMalloc((void**)&d_queue, 64));
    if (e == hipSuccess) e = hipMemcpy(d_rays, host_rays.data(), host_rays.size() * sizeof(float), hipMemcpyHostToDevice);
    // (on the ctx's stream, which the launch follows: it is a non-blocking stream, so a memset on the null stream -- asynchronous
    // for device memory -- could still be clearing these after the kernel has written them)
    if (e == hipSuccess) e = hipMemsetAsync(d_cand, 0, n_pad * words * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_hit, 0xFF, n_pad * 2 * sizeof(int32_t), c->stream);
    if (e != hipSuccess) { cleanup(); return fail(c, MRT_ERR_HIP, "mrt_debug_world_hit: %s failed: %s", what, hipGetErrorString(e)); }
    mrt::KParams p;
    std::memset(&p, 0, sizeof p);
    p.locals = c->locals;
    p.locals.shape[0] = 8; p.locals.shape[1] = (uint32_t)(n_rays / 8);
    p.locals.samples_per_frame = 1; p.locals.ray_depth = 1;
    fill_scene_params(c, p);
    p.shard_rank = 0; p.shard_world = 1;
    p.tiles_x = 1; p.n_tiles = (uint32_t)(n_rays / 64);
    p.tile_queue = d_queue;
    p.n_blocks = 1; p.pix_stride = 0; p.queue_layers = 1; p.lane_frames = 1;
    p.dbg_rays = d_rays; p.dbg_hit = d_hit; p.dbg_cand = d_cand; p.dbg_words = (uint32_t)words;
    p.counters = reinterpret_cast<unsigned long long*>(d_cand + n_rays * words);      // (n_rays x words x 4 bytes: a multiple of 256)
    int le = mrt::launch_debug_world_hit(p, c->n_waves, c->stream);
    int ws = MRT_OK;
    if (le == 0) ws = mrt::wait_stream(c, c->stream, "mrt_debug_world_hit");
    if (ws != MRT_OK) { cleanup(); return ws; }
    if (le != 0 || e != hipSuccess) { cleanup(); return fail(c, MRT_ERR_HIP, "mrt_debug_world_hit: launch failed: %s", hipGetErrorString(le ? (hipError_t)le : e)); }
    std::vector<int32_t> hits(n_pad * 2);
    e = hipMemcpy(hits.data(), d_hit, hits.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) std::memcpy(hit_out, hits.data(), n * 2 * sizeof(int32_t));
    if (e == hipSuccess && cand_out) {
        std::vector<uint32_t> cand(n_pad * words);
        e = hipMemcpy(cand.data(), d_cand, cand.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) {
            unsigned long long cnt[16];
            std::memcpy(cnt, cand.data() + n_rays * words, sizeof cnt);
            c->dbg_world_hit_stats[0] = cnt[1]; c->dbg_world_hit_stats[1] = cnt[4];
        }
        if (e == hipSuccess)
            for (size_t i = 0; i < n; i++) {
                std::memset(cand_out + i * cand_words, 0, cand_words * sizeof(uint32_t));
                std::memcpy(cand_out + i * cand_words, cand.data() + i * words, need_words * sizeof(uint32_t));
            }
    }
    cleanup();
    if (e != hipSuccess) return fail(c, MRT_ERR_HIP, "mrt_debug_world_hit: read-back failed: %s", hipGetErrorString(e));
    return MRT_OK;
}

int mrt_debug_set_boxes(mrt_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2) return MRT_ERR_INVALID_ARG;
    c->boxes_mode = mode;
    return MRT_OK;
}

int mrt_debug_sweep_variant(mrt_ctx* c) {
    if (!c || !c->have_world) return 0;
    return use_matrix_core_sweep(c) ? 2 : 1;
}

int mrt_debug_set_hierarchy(mrt_ctx* c, uint32_t max_levels, uint32_t top_target) {
    if (!c || max_levels < 1 || max_levels > mrt::kMaxLevels) return MRT_ERR_INVALID_ARG;      // top_target 0 = automatic
    c->max_levels = max_levels;
    c->top_target = top_target;
    return MRT_OK;
}

int mrt_debug_lds_layout(uint32_t n_members, uint32_t n_nodes, uint32_t levels, uint32_t n_top_padded, uint32_t out[3]) {
    if (!out || levels < 1 || levels > mrt::kMaxLevels) return MRT_ERR_INVALID_ARG;
    mrt::KParams p;
    std::memset(&p, 0, sizeof p);
    p.n_members = n_members; p.n_nodes = n_nodes; p.levels = levels; p.n_padded = n_top_padded;
    { const uint32_t ch = (n_top_padded + mrt::kChunk - 1) / mrt::kChunk; p.mask_chunks = ch < 16u ? ch : 16u; }
    p.box_lds_count = mrt::scene_is_small(n_members) ? 0u : mrt::large_scene_box_lds_count(n_top_padded, levels, p.mask_chunks, mrt::kBoxLdsCap);
    p.gen_cap = mrt::scene_is_small(n_members) ? mrt::kSmallGenCap : mrt::large_scene_stack_cap(p.mask_chunks, p.box_lds_count);
    uint32_t lay[2];
    mrt::render_lds_layout(p, lay);
    out[0] = lay[0]; out[1] = lay[1]; out[2] = p.gen_cap;
    return MRT_OK;
}

}  // extern "C"
