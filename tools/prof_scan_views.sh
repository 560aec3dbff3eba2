# kernel trace of tools/scan_views_time.py --trace: one call of each scanline form and two SMT_VIEW_BOTH pipeline calls
# under SMT_PIPE_SCHEDULE=2 at one size, in a process of its own; then tools/scan_views_overlap.py writes per-kernel
# durations and how much of every scanline launch ran beside an aggregation launch.
#     sh tools/prof_scan_views.sh [size, default hd] [out dir relative to the repository root, default prof_out/scan_views]
set -x
cd "$(dirname "$0")/.."
S=${1:-hd}
O=${2:-prof_out/scan_views}
mkdir -p $O
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$S -o s -- \
    python3 tools/scan_views_time.py --trace --sizes $S > $O/$S.out 2> $O/$S.err || exit 1
T=$(ls $O/$S/*kernel_trace.csv $O/$S/*/*kernel_trace.csv 2>/dev/null | head -1)
python3 tools/scan_views_overlap.py $T profiles/scan_views_trace_$S.json
