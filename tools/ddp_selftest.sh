# the data-parallel launch sequence of every bench leg on a 1-rank RCCL group; usage (repo root): bash tools/ddp_selftest.sh
# results and logs go to $OUT (default: a fresh temporary directory)
OUT=${OUT:-$(mktemp -d)}
export IB_DDP_SELFTEST=1
for extra in "--no-graph" "" "--overlap-comm on --bucket-mb 0.5" "--workload transformer_denoiser_T50 --steps 20 --warmup 3" "--workload transformer_denoiser_T50 --steps 20 --warmup 3 --overlap-comm off"; do
  timeout -k 10 200 python -X faulthandler bench.py --full --steps 60 --warmup 5 --no-cpu-baseline --no-ddim $extra > $OUT/ddp.json 2> $OUT/ddp.err; rc=$?
  echo "selftest [$extra] rc=$rc $(python -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(d['ms_per_step'], d['final_loss'], d['config']['grad_buckets'])" $OUT/ddp.json 2>/dev/null)"
  if [ $rc -ne 0 ]; then tail -c 1500 $OUT/ddp.err; fi
done
unset IB_DDP_SELFTEST
timeout -k 10 200 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --full --steps 60 --warmup 5 --no-cpu-baseline --no-ddim > $OUT/ddp_tr.json 2> $OUT/ddp_tr.err; echo "torchrun rc=$? $(tail -c 300 $OUT/ddp_tr.json | cut -c1-200)"
