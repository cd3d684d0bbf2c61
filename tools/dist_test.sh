#!/usr/bin/env bash
# Distributed evaluation (tools/dist_test.sh of the reference) on torch.distributed.run: one rank per GPU, each evaluating its shard.
# Usage: tools/dist_test.sh CONFIG CHECKPOINT GPUS [tools/test.py options]    (PORT: rendezvous port, default 29547)
CONFIG=$1
CHECKPOINT=$2
GPUS=$3
PORT=${PORT:-29547}
PYTHONPATH="$(dirname "$0")/..":$PYTHONPATH \
python -m torch.distributed.run --nnodes=1 --nproc-per-node="$GPUS" --master-addr 127.0.0.1 --master-port="$PORT" \
    "$(dirname "$0")/test.py" "$CONFIG" "$CHECKPOINT" --eval abs_rel --launcher pytorch "${@:4}"
