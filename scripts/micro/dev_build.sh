#!/bin/bash
# Dev tool: build experiment libraries of one kernel file (the compile-time stamp switches of csrc/dev.h,
# -DMDGEN_DEV_<PFX>_<NAME>) next to the product library.  From the repo root, no GPU needed:
#   bash scripts/micro/dev_build.sh STAMPS                          k_flash.hip, MDGEN_DEV_FLASH_STAMPS
#   KFILE=k_gemm KPFX=QKV  bash scripts/micro/dev_build.sh STAMPS   k_gemm.hip,  MDGEN_DEV_QKV_STAMPS
#   KFILE=k_gemm KPFX=MLP8 bash scripts/micro/dev_build.sh STAMPS   k_gemm.hip,  MDGEN_DEV_MLP8_STAMPS
# then:  MDGEN_AMD_LIB=build/dev_libs/libmdgen_amd_STAMPS.so python scripts/micro/flash_stamps.py ...
# Experiment libraries go to build/dev_libs/ (scratch, git-ignored).
set -e
cd "$(dirname "$0")/../.."
python -m mdgen_amd.build >/dev/null
mkdir -p build/dev_libs
KFILE=${KFILE:-k_flash}; KPFX=${KPFX:-FLASH}
EXTRA=""; [ $KFILE = k_flash ] && EXTRA="-fno-honor-nans"
# api.hip of every experiment library reports mdgen_dev_build() = 1 (csrc/dev.h)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -fno-slp-vectorize -Wno-unused-function \
    -Wno-pass-failed -DMDGEN_DEV_BUILD -c mdgen_amd/csrc/api.hip -o build/dev_libs/api_dev.o
for v in "$@"; do
  o=build/dev_libs/${KFILE}_$v.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -fno-slp-vectorize $EXTRA \
      -Wno-unused-function -Wno-pass-failed -DMDGEN_DEV_BUILD -DMDGEN_DEV_${KPFX}_$v -c mdgen_amd/csrc/$KFILE.hip -o $o
  objs=$(ls mdgen_amd/build/*.o | grep -v "/$KFILE.o" | grep -v "/api.o")
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/dev_libs/libmdgen_amd_$v.so $objs build/dev_libs/api_dev.o $o
  echo built build/dev_libs/libmdgen_amd_$v.so
done
