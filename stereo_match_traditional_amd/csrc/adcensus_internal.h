// Internal entry points of csrc/adcensus.hip shared with the other translation units of libsmt_hip.so (not exported,
// not part of include/smt.h).
#pragma once
#include "smt_common.h"

// The per-pair loop of smt_adcensus_compute_batch over pairs [0, n) of L / R ([n][H][W] each, maps likewise) on the
// handle's stream.  sched: how pairs b >= 1 get their tables -- 0 in order, 1 on the internal stream, 2 built inside
// the previous pair's launch (needs adcensus_fused_both_views and views == SMT_VIEW_BOTH), 3 as 2 in chains on internal
// streams joined before the return (include/smt.h; as 2 where n < 2, maps_ok is clear, prepped is set or nL / nR given).  prepped: pair 0's tables
// were built by the previous call's last launch (sched 2 with nL / nR).  nL, nR: with sched 2, the images of the pair
// after the last one, whose tables the last pair's launch builds (nullptr: none).  maps_ok: pairs may skip their
// volume stores (maps-only kernel); last_volumes: the last pair writes its volumes all the same.  The caller has
// checked the arguments and made the handle's device current.
int adcensus_batch_pairs(smt_adcensus *h, const float *L, const float *R, int n, int views, float *dispL,
                         float *dispR, int sched, bool prepped, const float *nL, const float *nR, bool maps_ok,
                         bool last_volumes);
// Both views of this handle take the register-window kernels (D <= 256), so sched 2 and the maps-only kernel apply.
bool adcensus_fused_both_views(const smt_adcensus *h);
