# kernel-trace stats of tools/sad_both_time.py at 1920x1080, D=128, 9x9: the tap-loop kernel of plain smt_sad (k_sad2<2>,
# one launch per view) beside what smt_sad_both launches (k_sad_box<2>, the key map's fill and k_sad_rkeys_finish; under
# impl 1 k_sad_box<2> with the volume store and k_sad_diag).
#     sh tools/prof_sad_both.sh [size, default hd] [out dir relative to the repository root, default prof_out/sad_both]
set -x
cd "$(dirname "$0")/.."
S=${1:-hd}
O=${2:-prof_out/sad_both}
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/s -o s -- \
    python3 tools/sad_both_time.py --sizes $S --rounds 1 --reps 2 --pairs 1 > $O/s.out 2> $O/s.err || exit 1
cp $(ls $O/s/*kernel_stats.csv $O/s/*/*kernel_stats.csv 2>/dev/null | head -1) $O/sad_both_kernel_stats.csv
