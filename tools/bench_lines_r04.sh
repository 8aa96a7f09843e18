#!/bin/bash
# The round's bench lines, one per BASELINE config, with the traffic file of the same kernel sources in place
# (tools/profile_round4.sh -> tools/collect_round4.sh first) -> profiles/bench_r04_config{1,2,3,4}.json (+ the saturating batch
# and the whole-utterance lines for comparison).  The config lines are --full ones (cpu_baseline, stream, end_to_end).
#   usage: tools/bench_lines_r04.sh OUTDIR
O=${1:?usage: tools/bench_lines_r04.sh OUTDIR}
cd ${GRAFT_REPO_ROOT:-.}
mkdir -p $O
python bench.py --full > $O/config1.json 2> $O/config1.err
for c in 2 3 4; do python bench.py --full --config $c > $O/config$c.json 2> $O/config$c.err; done
python bench.py --split off > $O/config1_whole.json 2>/dev/null
python bench.py --config 4 --split off > $O/config4_whole.json 2>/dev/null
python bench.py --voices 65536 --kernel wide > $O/wide65536.json 2>/dev/null
for f in $O/*.json; do python -c "import sys,json; d=json.loads(open(sys.argv[1]).read()); r=d['roofline']; print('%-22s %.3f ms  %.3e samples/s  frac %.4f  traffic %s  valu %s' % (sys.argv[1].split('/')[-1], d['ms_per_step'], d['value'], r['frac'], r['traffic'], (r['valu_issue'] or {}).get('frac_of_issue_slots')))" $f; done
