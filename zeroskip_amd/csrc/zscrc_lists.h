/*
 * zscrc_lists.h -- the record lists of a call as they lie on the device, for
 * the stages that take an array of zscrc_merge_list (the merge's lists, the
 * lookup's and the scan's levels): the descriptor the kernels read, the check
 * of the caller's array and the staging (both in zscrc_scratch.cpp).
 */
#ifndef ZSCRC_LISTS_H
#define ZSCRC_LISTS_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "../../include/zscrc.h"
#include "zscrc_internal.h"

namespace zsdev {

/* A list that is not empty: its records, the seq of its first one, its base.
 * The entry one past the last such list holds n_total. */
struct ListD {
    const zscrc_zs_record *recs;
    uint64_t first;
    uint64_t base;
};
struct Firsts {
    const ListD *d;
    __host__ __device__ uint64_t operator[](uint64_t i) const { return d[i].first; }
};

/* The caller's k <= kmax lists, N_MAX records in all; *n_total and *filled
 * (the lists that are not empty) on success. */
bool lists_ok(const zscrc_merge_list *lists, size_t k, size_t kmax, uint64_t *n_total, uint32_t *filled);
/* With sc.mu held: the descriptors of the `filled` lists that are not empty
 * and the entry that ends them to d_dst through the pinned staging. */
int stage_lists(zs::Scratch &sc, const zscrc_merge_list *lists, size_t k, uint32_t filled, ListD *d_dst,
                hipStream_t s);

} /* namespace zsdev */

#endif
