// volume_reentry_api.hip.h — the re-entry store of the moving TSDF volume (odo_volume_enable_reentry, _reentry_voxels, _reentry_stats,
// _reentry_time): the host side over the kernels of volume_reentry_kernels.hip. The voxels a shift pushes out of the window are kept
// with their global index, and every shift puts back those whose index lies inside the new window.
// Included by odometry_hip.hip behind volume_shift_api.hip.h, whose volume_shift enqueues the passes round the shift's launch.
//
// Nothing here waits for the device but the three readers and the timing. The store has two sets of buffers; a shift reads the live
// set and writes the second, and volume_shift swaps the pointers when it enqueues, as it swaps the grids.
#pragma once
#include "volume_reentry.hip.h"
#include "volume_shift_math.h"

// The passes' arguments for a shift by d that moves the window to off_new, from the volume as it is in front of the shift's swaps.
static VolReentryArgs volume_reentry_args(odo_volume* v, const int d[3], const int off_new[3]) {
  VolReentryArgs a;
  memset(&a, 0, sizeof(a));
  const bool store_colour = v->d_re_col != nullptr;
  a.old_vox = v->d_vox; a.old_col = v->colour ? v->d_col : nullptr;
  a.new_vox = v->d_vox2; a.new_col = store_colour ? v->d_col2 : nullptr;
  a.nx = v->p.nx; a.ny = v->p.ny; a.nz = v->p.nz; a.n = (int)v->n_vox;
  a.nblk = (int)((v->n_vox + kVolExtBlock - 1) / kVolExtBlock);
  a.dx = d[0]; a.dy = d[1]; a.dz = d[2];
  for (int c = 0; c < 3; c++) { a.off_old[c] = v->off[c]; a.off_new[c] = off_new[c]; }
  a.capacity = v->re_capacity;
  a.store_nblk = (int)((v->re_capacity + kVolExtBlock - 1) / kVolExtBlock);
  a.src = v->d_re_ent; a.src_col = v->d_re_col; a.dst = v->d_re_ent2; a.dst_col = v->d_re_col2;
  a.save_mask = v->d_re_save_mask; a.save_cnt = v->d_re_save_cnt; a.save_off = v->d_re_save_off;
  a.keep_mask = v->d_re_keep_mask; a.keep_cnt = v->d_re_keep_cnt; a.keep_off = v->d_re_keep_off;
  a.rc = v->d_re_ctr;
  return a;
}

// As the other two stores: every buffer of both sets has a guard of kSpillGuard entries behind the capacity and is filled with 0xAB
// once. The grids' second buffers and the passes' scratch are allocated here, so that no shift (no frame call of an attached tracker)
// allocates.
extern "C" int odo_volume_enable_reentry(odo_volume* v, long capacity) {
  const char* who = "odo_volume_enable_reentry";
  if (!v) return fail("%s: NULL volume", who);
  if (capacity < 1 || capacity > (1L << 28)) return fail("%s: capacity %ld out of range (1 .. 2^28)", who, capacity);
  if (v->re_capacity > 0) return fail("%s: the volume has a re-entry store already", who);
  if (v->attached) return fail("%s: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)", who);
  HIP_OK(hipSetDevice(v->device));
  if (volume_shift_buffers(who, v)) return -1;
  const size_t ne = (size_t)capacity;
  const size_t nblk = (size_t)((v->n_vox + kVolExtBlock - 1) / kVolExtBlock), sblk = (size_t)((capacity + kVolExtBlock - 1) / kVolExtBlock);
  const size_t waves = kVolExtBlock / 64;
  if (!volume_store_alloc(v, {{(void**)&v->d_re_ent, sizeof(uint4), ne, kGuarded},
                              {(void**)&v->d_re_ent2, sizeof(uint4), ne, kGuarded},
                              {v->colour ? (void**)&v->d_re_col : nullptr, sizeof(uint32_t), ne, kGuarded},
                              {v->colour ? (void**)&v->d_re_col2 : nullptr, sizeof(uint32_t), ne, kGuarded},
                              {(void**)&v->d_re_save_mask, sizeof(unsigned long long), waves * nblk, kPlain},
                              {(void**)&v->d_re_save_off, sizeof(unsigned long long), nblk, kPlain},
                              {(void**)&v->d_re_save_cnt, sizeof(unsigned), nblk, kPlain},
                              {(void**)&v->d_re_keep_mask, sizeof(unsigned long long), waves * sblk, kPlain},
                              {(void**)&v->d_re_keep_off, sizeof(unsigned long long), sblk, kPlain},
                              {(void**)&v->d_re_keep_cnt, sizeof(unsigned), sblk, kPlain},
                              {(void**)&v->d_re_ctr, sizeof(VolReentryCounters), 1, kZeroed},
                              {(void**)&v->d_re_ctr_time, sizeof(VolReentryCounters), 1, kZeroed}}))
    return fail("%s: device allocation failed (%ld entries)", who, capacity);
  v->re_capacity = capacity;
  return 0;
}

extern "C" int odo_volume_reentry_voxels(odo_volume* v, long capacity, int32_t (*g)[3], uint32_t* vox, uint32_t* col, long* n, int clear) {
  const char* who = "odo_volume_reentry_voxels";
  if (!v || !n || capacity < 0 || capacity > (1L << 28) || (capacity > 0 && (!g || !vox)))
    return fail("%s: bad arg (capacity 0 .. 2^28, buffers for `capacity` entries)", who);
  if (v->re_capacity <= 0) return fail("%s: the volume has no re-entry store (odo_volume_enable_reentry first)", who);
  if (col && !v->d_re_col) return fail("%s: the store has no colours (odo_volume_enable_colour before odo_volume_enable_reentry)", who);
  VolReentryCounters c;
  if (volume_read_counters(v, v->d_re_ctr, &c)) return -1;
  *n = (long)c.live;
  if (capacity > 0 && c.live > (unsigned long long)capacity)
    return fail("%s: the store holds %llu entries, the buffers %ld (nothing copied, nothing cleared; the count is returned)", who, c.live,
                capacity);
  const size_t m = (size_t)c.live;
  if (capacity > 0 && m > 0) {
    std::vector<uint4> host;
    try { host.resize(m); } catch (...) { return fail("out of memory"); }
    HIP_OK(hipMemcpyAsync(host.data(), v->d_re_ent, sizeof(uint4) * m, hipMemcpyDeviceToHost, v->own));
    if (col) HIP_OK(hipMemcpyAsync(col, v->d_re_col, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipStreamSynchronize(v->own));
    for (size_t e = 0; e < m; e++) {
      g[e][0] = (int32_t)host[e].x; g[e][1] = (int32_t)host[e].y; g[e][2] = (int32_t)host[e].z;
      vox[e] = host[e].w;
    }
  }
  if (clear) {
    HIP_OK(hipMemsetAsync(v->d_re_ctr, 0, sizeof(VolReentryCounters), v->own));
    if (volume_mark(v, v->own)) return -1;
  }
  return 0;
}

extern "C" int odo_volume_reentry_stats(odo_volume* v, long stats[4]) {
  const char* who = "odo_volume_reentry_stats";
  if (!v || !stats) return fail("%s: NULL arg", who);
  if (v->re_capacity <= 0) return fail("%s: the volume has no re-entry store (odo_volume_enable_reentry first)", who);
  VolReentryCounters c;
  if (volume_read_counters(v, v->d_re_ctr, &c)) return -1;
  stats[0] = (long)c.live; stats[1] = (long)c.saved; stats[2] = (long)c.restored; stats[3] = (long)c.dropped;
  return 0;
}

// Event timing of the passes for d, as odo_volume_shift_time times the shift's: batches of `reps` launches between events. Every pass
// writes scratch only: the grids' second buffers (the shift by d is enqueued first, so the restore finds what it would find), the
// store's second set, and a copy of the counters that the advance moves on instead of the store's own. Nothing is swapped in.
extern "C" int odo_volume_reentry_time(odo_volume* v, const int d[3], int reps, float us[5]) {
  const char* who = "odo_volume_reentry_time";
  if (!v || !d || !us) return fail("%s: NULL arg", who);
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  if (v->re_capacity <= 0) return fail("%s: the volume has no re-entry store (odo_volume_enable_reentry first)", who);
  if (v->attached) return fail("%s: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)", who);
  int off[3];
  if (volume_shift_window(who, v, d, off)) return -1;
  HIP_OK(hipSetDevice(v->device));
  if (volume_shift_buffers(who, v)) return -1;
  if (volume_order_on(v, v->own)) return -1;
  VolReentryArgs a = volume_reentry_args(v, d, off);
  a.rc = v->d_re_ctr_time;
  hipStream_t s = v->own;
  static const int order[5] = {0, 1, 3, 2, 4};   // (the shift's order: the scatter reads the store scan's `kept`)
  const auto stage = [&](int q) { launch_volume_reentry_stage(a, order[q], s); return true; };
  const auto warm = [&]() {
    const bool ok = hipMemcpyAsync(v->d_re_ctr_time, v->d_re_ctr, sizeof(VolReentryCounters), hipMemcpyDeviceToDevice, s) == hipSuccess;
    launch_volume_shift(volume_shift_args(v, d), s);
    for (int q = 0; q < 4; q++) stage(q);
    return ok;
  };
  float t[5];
  if (time_stages(who, s, reps, 5, t, warm, stage)) return -1;
  for (int q = 0; q < 5; q++) us[order[q]] = t[q];
  return volume_mark(v, s);
}

extern "C" int odo_debug_volume_reentry_guard(odo_volume* v, long* n_changed, long* n_guard) {
  const char* who = "odo_debug_volume_reentry_guard";
  if (!v || !n_changed || !n_guard) return fail("%s: NULL arg", who);
  if (v->re_capacity <= 0) return fail("%s: the volume has no re-entry store (odo_volume_enable_reentry first)", who);
  VolReentryCounters c;
  if (volume_read_counters(v, v->d_re_ctr, &c)) return -1;
  const size_t cap = (size_t)v->re_capacity, from = (size_t)std::min<unsigned long long>(c.live, (unsigned long long)cap);
  const size_t tail = cap + kSpillGuard - from, guard = (size_t)kSpillGuard;
  long bad[2] = {0, 0};
  // behind the live entries of the live set, then the guards of both sets
  if (volume_count_not_ab(v, {{v->d_re_ent + from, sizeof(uint4) * tail}, {v->d_re_col ? v->d_re_col + from : nullptr, sizeof(uint32_t) * tail}},
                          &bad[0]) ||
      volume_count_not_ab(v, {{v->d_re_ent + cap, sizeof(uint4) * guard}, {v->d_re_ent2 + cap, sizeof(uint4) * guard},
                              {v->d_re_col ? v->d_re_col + cap : nullptr, sizeof(uint32_t) * guard},
                              {v->d_re_col2 ? v->d_re_col2 + cap : nullptr, sizeof(uint32_t) * guard}}, &bad[1]))
    return -1;
  *n_changed = bad[0];
  *n_guard = bad[1];
  return 0;
}
