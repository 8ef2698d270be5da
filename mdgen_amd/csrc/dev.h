// dev.h -- the ONE place that knows the experiment switches of the kernels (included by common.h).
//
// Product builds (mdgen_amd/build.py) define none of them.  The experiment builds of scripts/micro/dev_build.sh pass
// -DMDGEN_DEV_BUILD together with the switch; a switch without it is a build error, so a stray -D cannot silently put
// stamp stores into a product library, and mdgen_dev_build() (api.hip) lets a loader see what a given .so was built with.
//
// A switch adds cycle stamps (stamp variables and stamp stores) to the product's code path and nothing else: a kernel
// has ONE code path.  Switches that changed what a kernel computes, loads, stores or schedules are retired; their
// results are recorded in profiles/r0*_experiments.txt, profiles/r02_flash_variants.txt and DESIGN.md.
//
//   MDGEN_DEV_FLASH_STAMPS      k_flash / k_flash_proj: per-wave s_memtime stamps (scripts/micro/flash_stamps.py, scripts/micro/fproj_stamps.py)
//   MDGEN_DEV_QKV_STAMPS        k_ln_qkv / k_ln_qkv_attn4: phase stamps         (scripts/micro/qkv_stamps.py, scripts/micro/attn4_stamps.py)
//   MDGEN_DEV_MLP8_STAMPS       k_mlp8: per-wave phase stamps held in SGPRs (scripts/micro/mlp8_stamps.py)
#pragma once

#if defined(MDGEN_DEV_FLASH_STAMPS) || defined(MDGEN_DEV_QKV_STAMPS) || defined(MDGEN_DEV_MLP8_STAMPS)
#ifndef MDGEN_DEV_BUILD
#error "an MDGEN_DEV_* experiment switch is set without -DMDGEN_DEV_BUILD: product libraries are built with none of them"
#endif
#define MDGEN_DEV_ANY 1
#endif
