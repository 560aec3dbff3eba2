# kernel-trace stats of tools/sad_subpixel_time.py: k_sad_refine_right beside k_sad_box<KT, true>, the key map's fill
# and k_sad_rkeys_finish (what smt_sad_both_subpixel launches in its default form), one size per run.
#     sh tools/prof_sad_subpixel.sh [size, default hd9] [out dir relative to the repository root, default prof_out/sad_subpixel]
set -x
cd "$(dirname "$0")/.."
S=${1:-hd9}
O=${2:-prof_out/sad_subpixel}
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$S -o s -- \
    python3 tools/sad_subpixel_time.py --sizes $S --rounds 2 --reps 2 --pairs 0 > $O/$S.out 2> $O/$S.err || exit 1
cp $(ls $O/$S/*kernel_stats.csv $O/$S/*/*kernel_stats.csv 2>/dev/null | head -1) $O/sad_subpixel_kernel_stats_$S.csv
