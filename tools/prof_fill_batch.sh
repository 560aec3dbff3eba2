# kernel-trace stats of tools/fill_time.py at 1920x1080, D=192, 8 pairs, in a run of its own: the kernels of the composed
# path (k_fill_collect, k_fill_apply, k_fill_count, k_fill_holes once per pair) beside the eight launches of
# smt_fill_the_hole_batch (k_fb_count, k_fb_collect x3, k_fb_apply x2, k_fb_holes, k_fb_writeback), the pipeline's
# kernels that produce the maps included.
#     sh tools/prof_fill_batch.sh [out dir relative to the repository root, default prof_out/fill_batch]
# leaves <out dir>/fill_batch_kernel_stats.csv (the committed copy: profiles/fill_batch_kernel_stats.csv)
set -x
cd "$(dirname "$0")/.."
O=${1:-prof_out/fill_batch}
mkdir -p $O
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/s -o s -- \
    python3 tools/fill_time.py --rounds 11 > $O/s.out 2> $O/s.err || exit 1
cp $(ls $O/s/*kernel_stats.csv $O/s/*/*kernel_stats.csv 2>/dev/null | head -1) $O/fill_batch_kernel_stats.csv
