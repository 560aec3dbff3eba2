# kernel-trace stats of tools/asw_both_time.py at config 4 (960x540, D=128, 35x35): the tap-loop kernel of plain smt_asw
# (k_asw3<2, 2, true, false>) beside the one smt_asw_both launches (k_asw3<2, 2, true, true>: the same tap loop + the
# rank keys), the key map's fill and finish, and the diagonal-gather kernel of impl 1.
#     sh tools/prof_asw_both.sh [out dir relative to the repository root, default prof_out/asw_both]
set -x
cd "$(dirname "$0")/.."
O=${1:-prof_out/asw_both}
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/s -o s -- \
    python3 tools/asw_both_time.py --sizes config4 --rounds 1 --reps 2 --pairs 1 > $O/s.out 2> $O/s.err || exit 1
cp $(ls $O/s/*kernel_stats.csv $O/s/*/*kernel_stats.csv 2>/dev/null | head -1) $O/asw_both_kernel_stats.csv
