"""Tables of the stream-order suite (tests/test_stream_order_gpu.py runs them on the device, tests/test_bounds_cpu.py
holds them to include/smt.h and to the bounds table where there is no device).  A plain module, importable without a GPU.

SYNCHRONISING   one decision per caller-buffer entry point (bounds_cases.REQUIRED and smt_ncc_flow_run_batch): ASYNC -- the entry returns while the
                caller's stream is still busy, which the device test observes -- or SYNC, for the entries whose comment in
                include/smt.h ends with the sentence "Synchronising.", or ASYNC_WARM, where the header excepts the first
                call on a handle in those words.  The CPU test reads the header both ways.
INT32_DECOY     the entries with int32 inputs, and why the tensor's own minimum is admissible at every position of each
                of them (what arena.Arena puts there until the inputs arrive).
NO_DECOY        {entry: {tensor: reason}} for inputs that have no admissible decoy and keep their data.  Empty today.
own_decoys()    the one input the rules leave equal to its data although a decoy exists (smt_sum_f32 of one element).
cases()         the table of bounds_cases.py outside HOST_ENTRIES, plus the environment sweeps of the two entries whose
                internal streams depend on it.
"""
import bounds_cases as BC

# torch.cuda._sleep cycles in front of every case.  It has to be a sleep that ends by itself: a kernel that waits for a
# host flag would be released only after the entry under test has returned, and an entry that synchronises (a correct
# one, smt_fill_the_hole, or a defective one) would then wait for a stream that waits for the host -- a hang, on a
# device that is shared.  Measured figures and the rule: the docstring of tests/test_stream_order_gpu.py.
DELAY = 400_000_000
DELAY_MS = 166.65 * DELAY / 400_000_000        # measured with events on the MI355X: 400e6 cycles last 166.65 ms

ASYNC, SYNC = "asynchronous", "Synchronising."
ASYNC_WARM = "a warm call neither allocates nor synchronises"      # the first call on a handle may wait, and the table's is one

# REQUIRED, and the entry that tests/ncc_box_cases.py registers into the bounds table when it is imported
SYNCHRONISING = {name: ASYNC for name in BC.REQUIRED + ["smt_ncc_flow_run_batch"]}
SYNCHRONISING.update({
    "smt_fill_the_hole": SYNC,                 # the third pass's list goes back to the host
    "smt_adcensus_option_aggregate": SYNC,     # owns and frees its aggregator inside the call
    "smt_remove_speckles": SYNC,               # the host iterates the label kernels on a device flag
    "smt_ncc_flow_run_batch": ASYNC_WARM,      # the handle's statistics tables grow to the largest batch seen; the warm
                                               # calls are those of test_ncc_chain
})

# Every loop these kernels run over such a value is bounded ABOVE by it, and the data are admissible at every position,
# so the minimum of the data is admissible everywhere (it is <= the value that stood there); it occurs in the data, so
# it also respects whatever lower bound the data respect.
INT32_DECOY = {
    "smt_crossarm_load_arm_maps": "k_load_arms clamps every length to 0..8191 and the aggregation clips a rectangle to the "
                                  "plane (and reports it through smt_crossarm_status)",
    "smt_cblsm_choose_arm_length": "k_choose_arm indexes rows i - up, up <= own[p], and i + dn, dn <= own[p]: the minimum is "
                                   "<= the arm of the first / last row, which stays inside; RL / RR / vert are only compared",
    "smt_cblsm_cost_aggregation_new": "cblsm_local_value skips rows outside the plane and clamps columns to 0..Wp; the arm "
                                      "volumes are counts >= 0, so the tap count L + R + 1 stays positive",
    "smt_cblsm_cost_aggregation_v4": "k_v4_literal clips every rectangle to the plane and flags it; an empty one is NaN",
    "smt_sad_crosscheck": "k_sad_crosscheck reads dR[p - dL[p]] only where that index is inside the map",
}

NO_DECOY = {}


def own_decoys(name, A):
    """{tensor: array} for the inputs of a case that the rules leave equal to their data although a decoy exists"""
    if name == "smt_sum_f32" and A._t["x"].data.size == 1:
        return {"x": A._t["x"].data + 1}            # one element has no reversal; any float is admissible in a sum
    return {}


def cases():
    """[(id, name, params, env)]: env is {} or the one variable the case runs under"""
    import ncc_box_cases  # noqa: F401  (registers smt_ncc_flow_run_batch; here, so that importing this module registers nothing)
    out = []
    for name in BC.ENTRIES:
        if name in BC.HOST_ENTRIES:
            continue
        sweep = [{}]
        plist = list(BC.CASES[name])
        if name == "smt_adcensus_compute_batch":
            sweep = [{"SMT_OVERLAP": v} for v in "012"]            # in order / internal stream / fused (read at every call)
        elif name in ("smt_pipeline_run_batch", "smt_pipeline_run_batch_post"):
            sweep = [{"SMT_PIPE_SCHEDULE": v} for v in "012"]      # read when the handle is created, inside the closure
        for env in sweep:
            for p in plist:
                tag = "".join(f"-{k}{v}" for k, v in env.items())
                out.append((f"{name}-{BC.case_id(p)}{tag}", name, p, env))
            if env.get("SMT_PIPE_SCHEDULE") == "2":
                # five pairs at the table's smallest shape: every event edge of the three-stream schedule (ev_scan and
                # ev_right of pair b - 2 are waited on from pair 2 on; tests/test_config_hashes_gpu.py says the same)
                p = dict(H=1, W=33, D=1, P=5)
                out.append((f"{name}-{BC.case_id(p)}-SMT_PIPE_SCHEDULE2", name, p, env))
    return out


# part two: the groups of fuzz_flow_cases.py that run as chains on reused handles.  Pipeline groups 4 .. 7 are the
# schedules unset / 0 / 1 / 2 (6 under QUIRK_FIX_RIGHT_ARM_STRIDE, 7 with the five-pair batch).
FLOW_GROUPS = dict(pipeline=(4, 5, 6, 7), cblsm=(0, 1), crossagg=(0, 1), sad=(0, 1), ncc=(0, 1), asw=(0, 1))
CHAIN = (0, 1, 2, 0)
WARM = 2
