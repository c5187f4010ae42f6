#!/bin/bash
# the N > 1 code path of bench.py with two ranks sharing the visible GPU (host-staged exchange: numbers not comparable);
# prints the bench line, then a summary of it
export MASTER_ADDR=127.0.0.1
LINE=$(timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 5 --warmup 2 --backend gloo --full --workload ${1:-quad1024_k2} | tail -1)
echo "$LINE"
echo "$LINE" | python -c '
import json, sys
d = json.loads(sys.stdin.read())
print("n_gpus", d["n_gpus"], d["config"]["workload"], d["config"]["mode"], "step %.3f ms" % d["ms_per_step"], "settle", d["settle"]["passes"], "exchange:", d["config"]["exchange"][:90])
print("same_step_one_gpu", d["same_step_one_gpu"], "exchange_checked", d.get("exchange_checked"), "stage_ms", d["stage_ms"])
'
