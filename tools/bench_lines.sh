#!/bin/bash
# the three bench lines again (TAG=r03e), once profiles/ holds this build's counter summaries (roofline.traffic / traffic_source)
cd "$(dirname "$0")/.."; out=${OUT_DIR:-profile_out}; mkdir -p "$out"
timeout 900 python3 bench.py --full --no-also > "$out/${TAG:-rXX}_bench.json" 2> "$out/${TAG:-rXX}_bench.err"
timeout 900 python3 bench.py --no-also --workload config3-fv4 > "$out/${TAG:-rXX}_fv4_bench.json" 2> /dev/null
timeout 900 python3 bench.py --no-also --workload config3-27pt > "$out/${TAG:-rXX}_27pt_bench.json" 2> /dev/null
tail -c 600 "$out/${TAG:-rXX}_bench.json"
