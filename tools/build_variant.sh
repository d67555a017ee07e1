#!/bin/bash
# usage: tools/build_variant.sh [UNIT.hip ...] NAME [-DFLAG ...]   -> athenak_amd/lib/variants/libakmi_NAME.so
# The units of the fused stage (athenak_amd/csrc/akmi_stage*.hip) are recompiled with the extra flags, at most 16 at a
# time; the other objects of the default build are reused.
#   * By default EVERY stage unit is recompiled: several of them read the macros of akmi_stage.hpp (AKMI_MF_BYTES,
#     AKMI_POW2DX, AKMI_ML) and the two march units share akmi_stage_march.hpp, so a -D flag that reached only one of them
#     would link a library whose units disagree.
#   * Leading arguments that end in .hip (or UNITS="a.hip b.hip") narrow that to the named units, the rest being taken
#     from the default build -- for a macro that one unit alone reads (AKMI_X12S_*, AKMI_CT_WAVES, AKMI_CKL, ... in
#     akmi_stage_mhd.hip; AKMI_C2P_PAIRS* in akmi_stage_c2p.hip; AKMI_HS2_WAVES in akmi_stage_hydro.hip).
#   -DAKMI_DEV_FAST restricts the scheme dispatch to PLM + HLLD/HLLC, ideal gas: seconds instead of minutes (all units).
#   AKMI_ISA=1 keeps each unit's device assembly as /tmp/akmi_var_NAME/UNIT-hip-amdgcn-amd-amdhsa-gfx950.s
set -e
units=$UNITS
while [ "${1%.hip}" != "$1" ]; do units="$units $1"; shift; done
name=$1; shift
root=$(cd $(dirname $0)/.. && pwd)
mkdir -p $root/athenak_amd/lib/variants /tmp/akmi_var_$name
cd $root/athenak_amd/csrc
[ -n "$units" ] || units=$(ls akmi_stage*.hip)
extra=""
[ -n "$AKMI_ISA" ] && extra="--save-temps=obj"
echo $units | tr ' ' '\n' | xargs -P 16 -I{} /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off \
  -fPIC -Wno-unused-value -mllvm -amdgpu-schedule-relaxed-occupancy=true $extra "$@" -c {} -o /tmp/akmi_var_$name/{}.o
objs=""
for o in $root/athenak_amd/lib/obj/*.o; do
  case " $units " in *" $(basename $o .o) "*) ;; *) objs="$objs $o";; esac
done
for u in $units; do objs="$objs /tmp/akmi_var_$name/$u.o"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $root/athenak_amd/lib/variants/libakmi_$name.so $objs -ldl
echo built $name
