// rtx_group.h -- a context that renders on several devices (rtx_group_create): what the entry points of rtx_api.cpp /
// rtx_post.hip / rtx_update.cpp call when the context they are handed is the root of a device group.
//
// One process, one member context (scene replica, streams, slab buffer) per logical rank, rank 0 = the root = the context
// the caller holds.  Frames shard by pixel rows -- rank g traces rows [g H / N, (g + 1) H / N) with the GLOBAL row index in ray
// generation (RayTracing.cu:12,16); a block of rows is one contiguous byte range of the frame (RayTracing.cu:238,457) --
// and the slabs are gathered into the root's device memory: grouped ncclSend / ncclRecv over xGMI (RCCL, ncclCommInitAll)
// or hipMemcpyPeerAsync; SURVEY.md 8(e).
#pragma once

#include "rtx_ctx.h"

#include <functional>

struct rtx_group; // defined in rtx_group.cpp

namespace rtxgroup {

// the group a context is the root of, or nullptr
inline rtx_group* of(const rtx_ctx* ctx) { return ctx ? ctx->group : nullptr; }

void destroy(rtx_group* g); // members other than the root, buffers, communicators (the root context is the caller's)

// scene edits and options, replicated: called by the root's entry point AFTER it has applied the call to itself
int scene_clear(rtx_ctx* root);
int scene_add_sphere(rtx_ctx* root, const float pos[3], float radius, const float rgb[3]);
int scene_add_plane(rtx_ctx* root, const float pos[3], const float normal[3], const float rgb[3], float width, float height);
int scene_set_sphere_motion(rtx_ctx* root, unsigned index, int mover, float speed);
int scene_set_lights(rtx_ctx* root, size_t n, const rtx_light* lights);
int scene_set_reflectivity(rtx_ctx* root, unsigned first, size_t n, const float* k); // (the root has validated and applied it)
int scene_set_patterns(rtx_ctx* root, size_t n, const rtx_pattern* patterns);        // (likewise, both)
int scene_set_object_pattern(rtx_ctx* root, unsigned first, size_t n, unsigned slot);
int scene_set_refraction(rtx_ctx* root, unsigned first, size_t n, const float* ior);
int scene_set_finish(rtx_ctx* root, unsigned first, size_t n, const rtx_finish* finishes);
int scene_set_shadow_casting(rtx_ctx* root, unsigned first, size_t n, const uint8_t* casts);
int scene_set_spots(rtx_ctx* root, size_t n, const rtx_spot* spots);
// edits in place (the root has validated the range and applied the edit to itself): the host form calls every member; the device
// form copies the rows from the root's device into every other member's scratch, behind `after` (an event on the caller's stream),
// and runs the kernel there -- logical ranks on the root's own GPU take the same path
int scene_set_spheres(rtx_ctx* root, unsigned first, size_t n, const float* rows);
int scene_set_spheres_device(rtx_ctx* root, unsigned first, size_t n, const float* d_rows, hipEvent_t after);
int scene_set_plane(rtx_ctx* root, unsigned index, const float pos[3], const float normal[3], const float rgb[3], float width, float height);
// a removal (the root has validated the set and compacted its own replica): every other member compacts its replica by the same
// ascending list of creation indices, from host memory
int scene_remove_objects(rtx_ctx* root, const std::vector<uint32_t>& ascending);
// before that, and before the root compacts: every other member allocates what its removal needs (rtx_remove_prepare)
int scene_remove_prepare(rtx_ctx* root, const std::vector<uint32_t>& ascending);
int set_option(rtx_ctx* root, int option, int64_t value);
int update_objects(rtx_ctx* root, double dt); // every member steps its own replica (the same arithmetic on the same values)

// The whole frame of `p`, sharded over the members, as RECORDS in d_out on the root's device (nullptr: the root's own frame
// buffer, with its zero-fill bookkeeping), complete in stream order on the root's stream.
int render_frame(rtx_ctx* root, const rtx_params* p, int mode, void* d_out, unsigned flags);
// n whole frames (rtx_submit_frames on a group): every rank traces its rows of all of them with one call, one gather per chunk.
int render_frames(rtx_ctx* root, size_t n, const rtx_params* params, int mode, void* const* d_outs, void* const* streams);
// ... as compact pixel words (W * H of them, include/rtx.h RTX_RENDER_COMPACT) in the group's word buffer on the root's device,
// complete in stream order on the root's stream; *d_words receives the buffer.  What rtx_update minimises from.
int render_words(rtx_ctx* root, const rtx_params* p, int mode, const uint32_t** d_words);


// fn(rank, member) for every rank: rank 0 on the caller's thread, the others on their submission threads where those are in use
// (RTX_OPT_GROUP_THREADS) -- and then a job may wait for its own device without holding the others up -- or one after the other.
// Returns when all have returned; the first failure by rank, reported on the root.
int run_on_ranks(rtx_ctx* root, const std::function<int(int, rtx_ctx*)>& fn);
bool threads_active(rtx_ctx* root); // the ranks other than the root have submission threads (started here if they are wanted and not yet running)
// Two phases on every rank, `queue` (device work) and `await` (waiting for it): with submission threads a rank does both in one go
// (the ranks wait side by side); on the caller's thread alone everything is queued first, so that the ranks' device work still
// overlaps, and then awaited on every rank -- also after a failure: nothing may still be running on a rank's buffers.
int run_phases(rtx_ctx* root, const std::function<int(int, rtx_ctx*)>& queue, const std::function<int(int, rtx_ctx*)>& await);
// rtx_update without a gather (RTX_OPT_GROUP_UPDATE): wanted for this group?  ... and what rtx_update.cpp reports back
bool update_direct_wanted(const rtx_ctx* root);
void update_direct_done(rtx_ctx* root, bool ok); // ok: counted; not ok: the group gathers on its root from now on

} // namespace rtxgroup
