// tests/cli_stub/tsar_stub.cpp plus the entries that only tsar_gipuma --geom_build_prior calls (host/tsar_gipuma.cpp refers to them
// weakly), for tests/test_cli_build_prior_cpu.py: recorded like the others; the stub's "device" memory is host memory.
#include "tsar_stub.cpp"

extern "C" {

void tsar_default_plane_prior_build_params(tsar_plane_prior_build_params* p) {
    trace("tsar_default_plane_prior_build_params", "");
    p->cell = 4;
    p->max_levels = 0;
}
int tsar_get_plane(tsar_ctx* ctx, float* planes, float* cost, int32_t* beview, float* ratio, int mem) {
    const int rc = trace("tsar_get_plane", "ctx=%d planes=%s cost=%s beview=%s ratio=%s mem=%d", ord(ctx), ps(planes), ps(cost), ps(beview), ps(ratio), mem);
    if (rc == TSAR_OK && cost)
        for (size_t p = 0; p < npix(ctx); p++) cost[p] = (float)(p % 7) * 0.125f;
    return rc;
}
int tsar_build_plane_prior(tsar_ctx* ctx, const float* depth, const float* score, int mem, const tsar_plane_prior_build_params* p, float* depth_out,
                           float* normal_world_out, uint8_t* level_out) {
    const int rc = trace("tsar_build_plane_prior", "ctx=%d depth=%s score=%s mem=%d cell=%d max_levels=%d depth_out=%s normal_world_out=%s level_out=%s", ord(ctx),
                         ps(depth), ps(score), mem, p->cell, p->max_levels, ps(depth_out), ps(normal_world_out), ps(level_out));
    if (rc != TSAR_OK) return rc;
    for (size_t q = 0; q < npix(ctx); q++) {
        if (depth_out) depth_out[q] = 2.0f;
        if (normal_world_out) { normal_world_out[3 * q] = 0.0f; normal_world_out[3 * q + 1] = 0.0f; normal_world_out[3 * q + 2] = -1.0f; }
        if (level_out) level_out[q] = 0;
    }
    return rc;
}

}   // extern "C"
