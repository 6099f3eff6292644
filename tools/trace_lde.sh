# usage: bash tools/trace_lde.sh [tag]: timeline of one batch of the D > 64 energy terms (bench.py's config4 block, D = 1024, 33 grid points),
# as built -> $VGPA_OUT/<tag>_lde_trace_D1024.txt (default out/)
export TMPDIR=/tmp
OUT=${VGPA_OUT:-out}; mkdir -p $OUT                       # VGPA_OUT: where the results go
TAG=${1:-r05}
export VGPA_HEAD=${VGPA_HEAD:-$(cat vgpa_amd/_tree.txt 2>/dev/null)}
rm -rf $OUT/tr_lde
rocprofv3 --kernel-trace -d $OUT/tr_lde -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-single-problem --no-config2 --no-config5 > $OUT/tr_lde.json 2> $OUT/tr_lde.err
DB=$(find $OUT/tr_lde -name "*results.db" | head -1)
{ echo "# tree $VGPA_HEAD"; python3 tools/trace_lde.py $DB -v; } > $OUT/${TAG}_lde_trace_D1024.txt
rm -rf $OUT/tr_lde
head -22 $OUT/${TAG}_lde_trace_D1024.txt
