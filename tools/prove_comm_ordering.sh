#!/bin/bash
# Shows that tests/test_gpu_comm_loopback.py::test_fused_step_ordering_* can catch a cross-stream ordering bug of the fused data-parallel
# step: builds two copies of the library with ONE event wait dropped in comm.hip (-DUBD_SABOTAGE_COMM=1: the communication stream
# does not wait for the gradients to be final; =2: the caller's stream does not wait for the reduced segment before Adam) and runs
# the ordering test against each (expected: FAILS) and against the product library (expected: passes).  GPU box only.
# Output: gpurun_out/comm_ordering_power.log
set -u
cd "$(dirname "$0")/.."
mkdir -p gpurun_out /tmp/sab_obj
bash tests/loopback/build.sh > /dev/null
for k in 1 2; do bash ubdvss_amd/csrc/build.sh variant comm_sab$k comm -DUBD_SABOTAGE_COMM=$k > /dev/null || exit 1; done
{
  echo "== communication stream does not wait for the final gradients (UBD_SABOTAGE_COMM=1): the ordering test is expected to FAIL =="
  UBD_LIB_PATH=tools/_ab/comm_sab1.so python -m pytest tests/test_gpu_comm_loopback.py -m gpu -q -k "fused_step_ordering" 2>&1 | tail -12
  echo "== caller's stream does not wait for the reduced segment before Adam (UBD_SABOTAGE_COMM=2): expected to FAIL =="
  UBD_LIB_PATH=tools/_ab/comm_sab2.so python -m pytest tests/test_gpu_comm_loopback.py -m gpu -q -k "fused_step_ordering" 2>&1 | tail -12
  echo "== product library: expected to pass =="
  python -m pytest tests/test_gpu_comm_loopback.py -m gpu -q 2>&1 | tail -5
} > gpurun_out/comm_ordering_power.log 2>&1
cat gpurun_out/comm_ordering_power.log
