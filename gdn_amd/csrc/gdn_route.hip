// The one kernel-family decision of the graph layer: the route table of include/gdn_hip.h as code.  Every staged entry
// point validates its arguments and switches on gdn_route; the host queries below are reads of it.  Host arithmetic
// only: the LDS budgets stay with the tile kernels (the gdn_tile_* predicates); each launcher keeps its own guard.
#include "gdn_common.hpp"

namespace {

// The diagnostic A/B overrides, each read once per process, here and nowhere else: GDN_FUSED_PATH=valu (no matrix-core
// kernel at any stage), GDN_BWD_PATH=valu (row-gather backward), GDN_BWD_SLICED=1 (d = 128 backward: always two slices)
bool env_valu(const char* name) { const char* e = getenv(name); return e && e[0] == 'v'; }
bool dense_allowed() { static const bool on = !env_valu("GDN_FUSED_PATH"); return on; }
bool dense_bwd_allowed() { static const bool on = !env_valu("GDN_BWD_PATH"); return on; }
bool bwd_sliced_forced() { return GDN_ENV_INT_ONCE("GDN_BWD_SLICED", 0) != 0; }

}  // namespace

int gdn_route(int stage, int n, int w, int d, int k, int flags, int* bwd_form) {
  const bool uses_w = stage == GDN_STAGE_PROJECT || stage == GDN_STAGE_PROJECT_BWD || stage == GDN_STAGE_TERMS ||
                      stage == GDN_STAGE_FUSED;
  const bool uses_k = stage == GDN_STAGE_AGGREGATE || stage == GDN_STAGE_ATTN_BWD || stage == GDN_STAGE_FUSED;
  if (!uses_w) w = 1;
  if (!uses_k) k = 1;
  // the supported shapes; no family beyond them
  if (n < 1 || n > 4096 || d < 1 || d > GDN_ANY_MAX_D || w < 1 || w > GDN_LONG_MAX_W || k < 1 || k > n || k + 1 > 1024)
    return GDN_FAMILY_NONE;
  const bool any = gdn_any_width(d), lng = w > GDN_MAX_W;
  const bool dense = !(flags & GDN_ROUTE_WIDE) && dense_allowed();   // the matrix-core kernels may be picked
  switch (stage) {
    case GDN_STAGE_PROJECT:
    case GDN_STAGE_AGGREGATE:
      if (flags & GDN_ROUTE_BF16)   // bf16 storage of x / xlin / z: matrix-core kernels only, no row-gather form
        return gdn_dense_supported(n, w, d, k) ? GDN_FAMILY_DENSE : GDN_FAMILY_NONE;
      if (any) return GDN_FAMILY_ANY;
      if (lng) return GDN_FAMILY_LONG;
      if (stage == GDN_STAGE_PROJECT && (flags & GDN_ROUTE_SERIES)) return GDN_FAMILY_LARGE;   // streaming rows
      if (dense && gdn_dense_supported(n, w, d, k)) return GDN_FAMILY_DENSE;
      return gdn_tile_forward_ok(stage, n, w, d, k, false) ? GDN_FAMILY_TILE : GDN_FAMILY_LARGE;
    case GDN_STAGE_ATTN_BWD: {
      if (any) return GDN_FAMILY_ANY;
      if (dense && dense_bwd_allowed() && gdn_dense_supported(n, 1, d, k)) return GDN_FAMILY_DENSE;
      const int form = gdn_tile_attn_bwd_form(n, d, k, bwd_sliced_forced());
      if (form < 0) return bwd_sliced_forced() && d == 128 ? GDN_FAMILY_NONE : GDN_FAMILY_LARGE;
      if (bwd_form) *bwd_form = form;
      return GDN_FAMILY_TILE;
    }
    case GDN_STAGE_PROJECT_BWD:
      if (any) return GDN_FAMILY_ANY;
      if (lng) return GDN_FAMILY_LONG;
      return gdn_tile_project_bwd_ok(n, w, d) ? GDN_FAMILY_TILE : GDN_FAMILY_NONE;
    case GDN_STAGE_TERMS: return lng ? GDN_FAMILY_LONG : any ? GDN_FAMILY_ANY : GDN_FAMILY_TILE;
    case GDN_STAGE_HEAD: return any ? GDN_FAMILY_ANY : GDN_FAMILY_TILE;
    case GDN_STAGE_FUSED:   // one launch, no workspace: the tile or nothing
      if (any || lng) return GDN_FAMILY_NONE;
      if (dense && gdn_dense_fused_supported(n, w, d, k)) return GDN_FAMILY_DENSE;
      return gdn_tile_forward_ok(stage, n, w, d, k, flags & GDN_ROUTE_SERIES) ? GDN_FAMILY_TILE : GDN_FAMILY_NONE;
  }
  return GDN_FAMILY_NONE;
}

extern "C" int gdn_kernel_family(int stage, int n, int w, int d, int k, int flags) {
  int form = 0;
  return gdn_route(stage, n, w, d, k, flags, &form) | form << 8;
}

// does the tile family run `stage`, the matrix-core kernels set aside (WIDE)?
static bool tile(int stage, int n, int w, int d, int k) {
  return gdn_route(stage, n, w, d, k, GDN_ROUTE_WIDE) == GDN_FAMILY_TILE;
}
// 1 when the one-launch fused forward (the window's tile in LDS) takes this shape
extern "C" int gdn_tile_fits(int n, int w, int d, int k) { return tile(GDN_STAGE_FUSED, n, w, d, k); }
int gdn_forward_staged_ok(int n, int w, int d, int k) {
  return tile(GDN_STAGE_PROJECT, n, w, d, k) && tile(GDN_STAGE_AGGREGATE, n, w, d, k);
}
// 1 when the tile kernels take every stage of a training step (harness.NativeTrainStep.applicable() asks)
extern "C" int gdn_train_supported(int n, int w, int d, int k) {
  return gdn_forward_staged_ok(n, w, d, k) && tile(GDN_STAGE_ATTN_BWD, n, w, d, k) && tile(GDN_STAGE_PROJECT_BWD, n, w, d, k);
}
// 0 where the matrix-core backward runs, which does not read the reverse lists (rent / rlen may then be null)
extern "C" int gdn_attn_aggregate_bwd_uses_reverse(int n, int d, int k) {
  return gdn_route(GDN_STAGE_ATTN_BWD, n, 1, d, k, 0) != GDN_FAMILY_DENSE;
}
