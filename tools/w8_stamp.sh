#!/bin/bash
# s_memtime stamps of the 256x256 weight-gradient loop (UNIT_W8_STAMP, csrc/conv_wgrad256p8.hip): `tools/w8_stamp.sh build` where hipcc is,
# `tools/w8_stamp.sh` on the GPU box (prints the table of tools/w8_stamp.py)
if [ "$1" = build ]; then
  python3 -c "import __graft_entry__ as g; g.build()"
  mkdir -p unit_amd/_build/w8stamp
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -ffp-contract=off -std=c++17 -Wno-unused-value -DUNIT_W8_STAMP=1 -c unit_amd/csrc/conv_wgrad256p8.hip -o unit_amd/_build/w8stamp/w8.o || exit 1
  objs=$(ls unit_amd/_build/*.o | grep -v conv_wgrad256p8.o)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o unit_amd/_build/w8stamp/libunit_hip.so $objs unit_amd/_build/w8stamp/w8.o || exit 1
  exit 0
fi
export UNIT_HIP_LIB=$PWD/unit_amd/_build/w8stamp/libunit_hip.so
python3 tools/w8_stamp.py
