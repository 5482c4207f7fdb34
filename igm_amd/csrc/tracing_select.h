// The keep_best selection of the tracing A-steps (tracing_assign.hip), callable from every entry
// that ranks rows of f32 costs: per row the kb smallest of its N costs in increasing order, ties
// to the lower index -- the LDS sort up to its limit, the counting pass beyond it.
#pragma once
#include "igm_ctx.h"

namespace igm {

// cost (rows, N) f32 (>= 0 or +inf, never NaN) -> best_cand, best_cost (rows, kb), on c->stream
int tracing_select(igm_ctx* c, const float* cost, int rows, int N, int kb, int* best_cand, float* best_cost);

}  // namespace igm
