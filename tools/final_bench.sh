set -x
cd $GRAFT_REPO_ROOT
O=${BENCH_OUT:-bench_out}; mkdir -p $O
python bench.py --full > $O/r06_final_bench.json 2> $O/r06_final_bench.err
python bench.py --full --grch38-like --no-cpu --no-secondary > $O/r06_final_grch38_like_pe.json 2>> $O/r06_final_bench.err
python bench.py --full --grch38-like --se --no-cpu --no-secondary > $O/r06_final_grch38_like_se.json 2>> $O/r06_final_bench.err
python bench.py --full --grch38-like --sensitive --units 5000000 --no-cpu --no-secondary > $O/r06_final_grch38_like_sensitive.json 2>> $O/r06_final_bench.err
tail -c 600 $O/r06_final_bench.json
