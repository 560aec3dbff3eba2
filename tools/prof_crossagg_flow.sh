# kernel-trace stats of tools/crossagg_flow_time.py at 1280x720 D=128 (8 pairs, composed and fused form side by side):
# the fused first pass (k_caf_first) against what it replaces (k_cblsm_ad + the first horizontal k_ca_pass2), and the
# dividing pass with the WTA (k_ca_pass2_wta) against k_ca_pass2 + k_wta.
#     sh tools/prof_crossagg_flow.sh [out dir relative to the repository root, default prof_out/crossagg_flow]
set -x
cd "$(dirname "$0")/.."
O=${1:-prof_out/crossagg_flow}
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/s -o s -- \
    python3 tools/crossagg_flow_time.py --sizes 720p --samples 3 > $O/s.out 2> $O/s.err || exit 1
cp $(ls $O/s/*kernel_stats.csv $O/s/*/*kernel_stats.csv 2>/dev/null | head -1) $O/crossagg_flow_kernel_stats.csv
