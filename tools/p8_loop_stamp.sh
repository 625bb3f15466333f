#!/bin/bash
# s_memtime stamps of the 256x256 forward tile's main loop (UNIT_EPI_STAMP, csrc/conv_igemm256p8.hip): `tools/p8_loop_stamp.sh build` where hipcc
# is, `tools/p8_loop_stamp.sh [variant ...]` on the GPU box (prints the table of tools/p8_loop_stamp.py). The build is tools/epi_stamp.sh's.
if [ "$1" = build ]; then
  exec "$(dirname "$0")/epi_stamp.sh" build
fi
export UNIT_HIP_LIB=$PWD/unit_amd/_build/epistamp/libunit_hip.so
python3 tools/p8_loop_stamp.py "$@"
