#!/bin/bash
# headline step + per-class times, nothing else
cd "$(dirname "$0")/../.." && python bench.py --full --windows 7 --no-extras --no-cpu-baseline 2>&1 | tail -1 | python -c "
import json, sys; r = json.loads(sys.stdin.read()); print(r['value'], r['ms_per_step'], r['kernel_class_ms_per_step'])"
