// rg_pcm_seam.h -- internal, HIP only: what the test seams that take tracks in a host arena on three routes (rg_pcm_stats_arena,
// rg_spectrum_arena, rg_dr_arena, rg_stereo_arena, rg_ancestry_arena, rg_rip_checksums_arena) have in common.  Route 0 and route 2 are the
// scan's host routes and need no context; route 1 copies the arena to the device and runs the kernels there.
#pragma once

#include <new>

#include "rg_ctx.h"
#include "rg_pcm_plane.h"

// The seam called `name` (`route2`: what it calls route 2, "folded").  host(err, err_len) is routes 0 and 2 as a whole.  Route 1:
// plan(err, err_len) checks the options and the descriptors and builds what the launch takes, with no device yet; then the
// arena goes up on the first slot's stream `s`, into whole 16-byte words (the staging's aligned cover), and device(c, s) launches
// and fills the records.  host and plan leave their text in err; device sets the context's error itself.
template <typename Host, typename Plan, typename Device>
int rg_pcm_arena_seam(void *ctx, int route, const char *name, const char *route2, size_t n, const void *descs, const void *out, const void *arena,
                      size_t arena_bytes, Host host, Plan plan, Device device) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    char err[256] = "";
    if (!c && route == 1) return RG_ERR_INVALID_ARG;  // the host routes need no context (their error text: rg_last_error(NULL))
    if (route < 0 || route > 2)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "%s: route %d (0 = serial host twin, 1 = kernels, 2 = %s on the host)", name, route, route2);
    if (rg_pcm_check_arrays(name, n, descs, out, arena, arena_bytes, err, sizeof err) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "%s", err);
    try {
        int rc = route != 1 ? host(err, sizeof err) : plan(err, sizeof err);
        if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
        if (route != 1) return RG_OK;
        rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        RG_HIP(c, c->d_arena.reserve(((arena_bytes + 15) & ~(size_t)15) + 16));
        hipStream_t s = c->slots[0].stream;
        if (arena_bytes) RG_HIP(c, hipMemcpyAsync(c->d_arena.p, arena, arena_bytes, hipMemcpyHostToDevice, s));
        return device(c, s);
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}
