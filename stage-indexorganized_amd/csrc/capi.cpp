// capi.cpp -- the extern "C" boundary (include/stage_hip.h).  No exception crosses it.
#include <hip/hip_runtime_api.h>

#include <execinfo.h>
#include <unistd.h>

#include <csignal>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "handle.hpp"

namespace stage_capi {
thread_local std::string g_err;
}
using namespace stage_capi;

extern "C" {

const char *stage_last_error(void) { return g_err.c_str(); }

// STAGE_SEGV_TRACE=1: a host-side SIGSEGV / SIGABRT prints the native backtrace of the faulting
// thread to stderr before the default action (host-code debugging on the GPU box, where no
// debugger is available)
namespace {
void segv_trace(int sig) {
    void *frames[64];
    const int n = backtrace(frames, 64);
    const char msg[] = "stage: fatal signal, native backtrace:\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    backtrace_symbols_fd(frames, n, 2);
    std::signal(sig, SIG_DFL);
    raise(sig);
}
struct SegvTraceInit {
    SegvTraceInit() {
        if (std::getenv("STAGE_SEGV_TRACE")) {
            std::signal(SIGSEGV, segv_trace);
            std::signal(SIGABRT, segv_trace);
        }
    }
} segv_trace_init;
}  // namespace
const char *stage_version(void) { return "stage-hip 0.1 (gfx950)"; }

int stage_table_create(const stage_params *params, stage_table **out) {
    if (!params || !out) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        auto t = std::make_unique<stage_table>();
        t->host = std::make_unique<stage::HostTable>(*params);
        t->dev.device = params->device;
        if (const char *g = std::getenv("STAGE_OUT_STRIDE")) {
            uint32_t v = (uint32_t)std::atoi(g);
            if (v >= ((t->host->key_pad() + t->host->params().payload_size + 15) & ~15u) && v % 16 == 0)
                t->out_stride = v;
        }
        *out = t.release();
        return STAGE_OK;
    });
}

int stage_table_destroy(stage_table *t) {
    if (!t) return STAGE_OK;
    return guarded([&] {
        if (t->dev.stream) (void)hipSetDevice(t->dev.device);
        delete t;
        return STAGE_OK;
    });
}

int stage_insert(stage_table *t, uint64_t key, uint16_t key_size, const uint8_t *payload, uint64_t gen_rowid,
                 int payload_mode, uint32_t commit_id, uint8_t *rc_out) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return guarded([&] {
        int rc = host(t).insert(key, key_size, payload, gen_rowid, payload_mode, commit_id);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_load_ycsb(stage_table *t, uint64_t begin_rowid, uint64_t end_rowid, uint32_t key_size, int payload_mode,
                    uint64_t *inserted) {
    if (!t || key_size == 0 || key_size > 8) return fail(STAGE_E_ARG, "bad arguments");
    return guarded([&] {
        uint64_t n = host(t).load_ycsb(begin_rowid, end_rowid, key_size, payload_mode);
        if (inserted) *inserted = n;
        return STAGE_OK;
    });
}

int stage_load_keys(stage_table *t, const uint64_t *keys, uint64_t n, uint32_t key_size, int payload_mode,
                    uint64_t *inserted) {
    if (!t || (!keys && n) || key_size == 0 || key_size > 8) return fail(STAGE_E_ARG, "bad arguments");
    return guarded([&] {
        uint64_t c = host(t).load_keys(keys, n, key_size, payload_mode);
        if (inserted) *inserted = c;
        return STAGE_OK;
    });
}

int stage_update(stage_table *t, uint64_t key, uint16_t key_size, uint32_t payload_off, const uint8_t *delta,
                 uint32_t delta_len, uint32_t writer_id, uint8_t *rc_out) {
    if (!t || (!delta && delta_len)) return fail(STAGE_E_ARG, "bad arguments");
    return guarded([&] {
        ensure_host_rows(t);
        int rc = host(t).update(key, key_size, payload_off, delta, delta_len, writer_id);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_commit_update(stage_table *t, uint64_t key, uint16_t key_size, uint32_t commit_id, uint32_t sstamp,
                        uint8_t *rc_out) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return guarded([&] {
        int rc = host(t).commit_update(key, key_size, commit_id, sstamp);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_update_batch(stage_table *t, const void *keys, uint32_t key_stride, uint64_t n, uint16_t key_size,
                       uint32_t payload_off, const uint8_t *deltas, uint32_t delta_len, const uint32_t *writer_ids,
                       const uint32_t *commit_ids, const uint32_t *sstamps, uint8_t *rc_out, uint64_t *n_ok) {
    if (!t || (n && (!keys || !writer_ids || (!deltas && delta_len))) || key_stride < key_size)
        return fail(STAGE_E_ARG, "bad arguments");
    return guarded([&] {
        ensure_host_rows(t);
        uint64_t ok = host(t).update_batch((const uint8_t *)keys, key_stride, n, key_size, payload_off, deltas,
                                            delta_len, writer_ids, commit_ids, sstamps, rc_out);
        if (n_ok) *n_ok = ok;
        return STAGE_OK;
    });
}

int stage_finalize_update(stage_table *t, uint64_t key, uint16_t key_size, uint32_t commit_id, uint8_t *rc_out) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return guarded([&] {
        int rc = host(t).finalize_update(key, key_size, commit_id);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_delete(stage_table *t, uint64_t key, uint16_t key_size, uint32_t commit_id, uint8_t *rc_out) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return guarded([&] {
        int rc = host(t).remove(key, key_size, commit_id);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

// ---- byte-key forms (any key width of the table, up to 32 bytes)
int stage_insert_key(stage_table *t, const uint8_t *key, uint16_t key_size, const uint8_t *payload, uint32_t commit_id,
                     uint8_t *rc_out) {
    if (!t || !key || !payload) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        int rc = host(t).insert(key, key_size, payload, 0, 0, commit_id);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_insert_key_inflight(stage_table *t, const uint8_t *key, uint16_t key_size, const uint8_t *payload,
                              uint32_t writer_id, uint8_t *rc_out) {
    if (!t || !key || !payload) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        int rc = host(t).insert(key, key_size, payload, 0, 0, writer_id, true);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_commit_insert_key(stage_table *t, const uint8_t *key, uint16_t key_size, uint32_t commit_id,
                            uint8_t *rc_out) {
    if (!t || !key) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        int rc = host(t).commit_insert(key, key_size, commit_id);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_load_rows(stage_table *t, const uint8_t *keys, uint32_t key_stride, uint16_t key_size,
                    const uint8_t *payloads, uint32_t payload_stride, uint64_t n, uint32_t commit_id,
                    uint8_t *rc_out, uint64_t *inserted) {
    if (!t || (n && (!keys || !payloads)) || key_stride < key_size) return fail(STAGE_E_ARG, "bad arguments");
    if (payload_stride < host(t).params().payload_size) return fail(STAGE_E_ARG, "payload stride < payload size");
    return guarded([&] {
        uint64_t c = host(t).load_rows(keys, key_stride, key_size, payloads, payload_stride, n, commit_id, rc_out);
        if (inserted) *inserted = c;
        return STAGE_OK;
    });
}

int stage_update_key(stage_table *t, const uint8_t *key, uint16_t key_size, uint32_t payload_off,
                     const uint8_t *delta, uint32_t delta_len, uint32_t writer_id, uint8_t *rc_out) {
    if (!t || !key || (!delta && delta_len)) return fail(STAGE_E_ARG, "bad arguments");
    return guarded([&] {
        ensure_host_rows(t);
        int rc = host(t).update(key, key_size, payload_off, delta, delta_len, writer_id);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_commit_update_key(stage_table *t, const uint8_t *key, uint16_t key_size, uint32_t commit_id,
                            uint32_t sstamp, uint8_t *rc_out) {
    if (!t || !key) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        int rc = host(t).commit_update(key, key_size, commit_id, sstamp);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_update_key_owned(stage_table *t, const uint8_t *key, uint16_t key_size, uint32_t payload_off,
                           const uint8_t *delta, uint32_t delta_len, uint32_t writer_id, uint8_t *rc_out) {
    if (!t || !key || (!delta && delta_len)) return fail(STAGE_E_ARG, "bad arguments");
    return guarded([&] {
        ensure_host_rows(t);
        int rc = host(t).update_owned(key, key_size, payload_off, delta, delta_len, writer_id);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_delete_key_owned(stage_table *t, const uint8_t *key, uint16_t key_size, uint8_t *rc_out) {
    if (!t || !key) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        int rc = host(t).remove_owned(key, key_size);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_delete_key(stage_table *t, const uint8_t *key, uint16_t key_size, uint32_t commit_id, uint8_t *rc_out) {
    if (!t || !key) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        int rc = host(t).remove(key, key_size, commit_id);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_abort_update_key(stage_table *t, const uint8_t *key, uint16_t key_size, uint8_t *rc_out) {
    if (!t || !key) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        int rc = host(t).abort_update(key, key_size);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_abort_insert_key(stage_table *t, const uint8_t *key, uint16_t key_size, uint8_t *rc_out) {
    if (!t || !key) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        int rc = host(t).abort_insert(key, key_size);
        if (rc_out) *rc_out = (uint8_t)rc;
        return STAGE_OK;
    });
}

int stage_settle(stage_table *t) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return guarded([&] {
        t->settle();
        return STAGE_OK;
    });
}

uint32_t stage_key_words(stage_table *t) { return t ? facts(t).key_words() : 0; }

int stage_sync(stage_table *t) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return guarded([&] {
        stage::sync_device(host(t), t->dev);
        return STAGE_OK;
    });
}

int stage_sync_info(stage_table *t, double *seconds, uint64_t *info) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    if (seconds) *seconds = t->dev.last_sync_seconds;
    if (info) {
        info[0] = t->dev.last_sync_incremental ? 1 : 0;
        info[1] = t->dev.last_patch_leaves;
        info[2] = t->dev.last_patch_slots;
    }
    return STAGE_OK;
}

int stage_stats(stage_table *t, uint64_t *stats) {
    if (!t || !stats) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        host(t).stats(stats);
        return STAGE_OK;
    });
}

uint32_t stage_record_stride(stage_table *t) { return t ? (t->out_stride ? t->out_stride : facts(t).stride()) : 0; }
uint32_t stage_leaf_capacity(stage_table *t) { return t ? facts(t).cap() : 0; }

int stage_traverse_batch(stage_table *t, const uint64_t *keys, const uint16_t *lens, uint64_t n, int le_child,
                         uint32_t *leaf_out) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    if ((!keys || !leaf_out) && n) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        // leaf index in key order: from the published image, or recomputed if host writes
        // happened since (the traversal itself never needs the device)
        std::vector<uint32_t> local;
        const std::vector<uint32_t> *map = &t->dev.host_to_dev;
        if (!t->dev.valid || host(t).layout_dirty_) {
            std::vector<uint32_t> order;
            host(t).key_order(order);
            local.assign(host(t).leaves_.size(), 0xFFFFFFFFu);
            for (size_t i = 0; i < order.size(); ++i) local[order[i]] = (uint32_t)i;
            map = &local;
        }
        const uint32_t width = host(t).params().key_width, kwords = host(t).key_words();
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t len = width ? width : (lens ? lens[i] : 8u);
            const stage::Key k = host(t).key_of(reinterpret_cast<const uint8_t *>(keys + i * kwords), len);
            leaf_out[i] = (*map)[host(t).route(k, le_child != 0)];
        }
        return STAGE_OK;
    });
}

int64_t stage_export_leaves(stage_table *t, uint32_t cap, uint64_t max_leaves, uint32_t *rc, uint32_t *sc,
                            uint64_t *meta, uint64_t *keyw) {
    if (!t || !rc || !sc || !meta || !keyw || cap == 0) return fail(STAGE_E_ARG, "null argument");
    try {
        const int64_t n = host(t).export_leaves(cap, max_leaves, rc, sc, meta, keyw);
        if (n < 0) return fail(STAGE_E_ARG, "max_leaves is smaller than the leaf count (stage_stats[2])");
        return n;
    } catch (const std::bad_alloc &) {
        return fail(STAGE_E_NOMEM, "host allocation failed");
    } catch (const std::exception &e) {
        return fail(STAGE_E_HIP, e.what());
    }
}

int64_t stage_export_leaf_images(stage_table *t, uint64_t max_leaves, uint8_t *blocks, uint64_t *sep_keys,
                                 uint16_t *sep_lens) {
    if (!t || !blocks || (!sep_keys != !sep_lens)) return fail(STAGE_E_ARG, "bad arguments");
    try {
        ensure_host_rows(t);
        const int64_t n = host(t).export_leaf_images(max_leaves, blocks, sep_keys, sep_lens);
        if (n < 0) return fail(STAGE_E_ARG, "max_leaves is smaller than the leaf count (stage_stats[2])");
        return n;
    } catch (const std::bad_alloc &) {
        return fail(STAGE_E_NOMEM, "host allocation failed");
    } catch (const std::exception &e) {
        return fail(STAGE_E_HIP, e.what());
    }
}

int64_t stage_export_locations(stage_table *t, uint64_t max, uint64_t *handles, uint32_t *leaf, uint16_t *slot) {
    if (!t || (max && (!handles || !leaf || !slot))) return fail(STAGE_E_ARG, "bad arguments");
    try {
        return (int64_t)host(t).export_locations(max, handles, leaf, slot);
    } catch (const std::bad_alloc &) {
        return fail(STAGE_E_NOMEM, "host allocation failed");
    } catch (const std::exception &e) {
        return fail(STAGE_E_HIP, e.what());
    }
}

int stage_resolve_locations(stage_table *t, const uint64_t *handles, uint64_t n, uint32_t *leaf, uint16_t *slot) {
    if (!t || (n && (!handles || !leaf || !slot))) return fail(STAGE_E_ARG, "bad arguments");
    return guarded([&] {
        host(t).resolve_locations(handles, n, leaf, slot);
        return STAGE_OK;
    });
}

// ---- what the kept transaction manager reads through a Record (stage_hip.h) ----------------

}  // extern "C"

// the SSN state of copy `id` under its mutex; a copy the device wrote in an epoch the host has
// not adopted yet is waited for (stage_table::settle) once
template <class F>
static int with_copy(stage_table *t, uint32_t id, F fn) {
    stage::CopySsnTable &s = t->host->ssn_;
    {
        std::unique_lock<std::mutex> g(s.mu);
        if (id < s.e.size()) return fn(s, s.e[id]);
    }
    int rc = guarded([&] {
        t->settle();
        return STAGE_OK;
    });
    if (rc) return rc;
    std::unique_lock<std::mutex> g(s.mu);
    if (id >= s.e.size()) return fail(STAGE_E_ARG, "no such overwrite copy");
    return fn(s, s.e[id]);
}

extern "C" {

int stage_probe_identify(stage_table *t, const stage_probe_out *d_out, uint64_t n, stage_probe_ident *d_ident,
                      void *stream) {
    int rc = need_synced(t);
    if (rc) return rc;
    if (n && (!d_out || !d_ident)) return fail(STAGE_E_ARG, "null device buffer");
    if (t->status_bytes != 32) return fail(STAGE_E_STATE, "stage_probe_identify reads 32-B status records (leaf, slot)");
    hipError_t e = hipSetDevice(t->dev.device);
    if (e != hipSuccess) return hip_rc(e, "hipSetDevice");
    e = stage::launch_ident(t->dev.view, reinterpret_cast<const stage::stage_probe_out_dev *>(d_out), n,
                            reinterpret_cast<uint32_t *>(d_ident), pick(t, stream));
    return hip_rc(e, "ident kernel");
}

int stage_record_meta_key(stage_table *t, const uint8_t *key, uint16_t key_size, uint64_t *meta,
                          stage_probe_ident *ident, uint8_t *rc_out) {
    if (!t || !key || !meta || !ident) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] {
        stage::HostTable &h = host(t);
        uint32_t leaf, slot;
        *meta = 0;
        *ident = stage_probe_ident{0, 0};
        if (h.find(key, key_size, &leaf, &slot) < 0) {
            if (rc_out) *rc_out = STAGE_RC_NOT_FOUND;
            return STAGE_OK;
        }
        const size_t i = (size_t)leaf * h.cap() + slot;
        *meta = h.meta_[i];
        *ident = stage_probe_ident{h.loc_[i], h.next_[i]};
        if (rc_out) *rc_out = STAGE_RC_OK;
        return STAGE_OK;
    });
}

int stage_location_cells(stage_table *t) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return guarded([&] {
        host(t).enable_cells();
        return STAGE_OK;
    });
}

int stage_location_cell(stage_table *t, uint64_t handle, const void **cell) {
    if (!t || !cell) return fail(STAGE_E_ARG, "null argument");
    stage::HostTable &h = *t->host;  // no settle: a cell is read while the writer goes on
    if (!h.cells_.on()) return fail(STAGE_E_STATE, "location cells are off: call stage_location_cells first");
    if (handle == 0 || (handle >> stage::LocCells::kChunkBits) >= stage::LocCells::kDir)
        return fail(STAGE_E_ARG, "location handle out of range");
    return guarded([&] {
        h.cells_.ensure(handle);
        *cell = h.cells_.find(handle);
        return STAGE_OK;
    });
}

int stage_copy_get(stage_table *t, const uint32_t *copy_ids, uint64_t n, stage_copy_state *out) {
    if (!t || (n && (!copy_ids || !out))) return fail(STAGE_E_ARG, "bad arguments");
    for (uint64_t i = 0; i < n; ++i) {
        const int rc = with_copy(t, copy_ids[i], [&](stage::CopySsnTable &s, stage::CopySsn &c) {
            auto it = s.readers.find(copy_ids[i]);
            out[i] = stage_copy_state{c.cstamp, c.pstamp, c.rstamp, c.sstamp,
                                      it == s.readers.end() ? 0u : (uint32_t)it->second.size(), c.count, c.waiting, 0};
            return STAGE_OK;
        });
        if (rc) return rc;
    }
    return STAGE_OK;
}

int stage_copy_readers(stage_table *t, uint32_t copy_id, uint32_t *read_ids, uint32_t max, uint32_t *count) {
    if (!t || !count || (max && !read_ids)) return fail(STAGE_E_ARG, "bad arguments");
    return with_copy(t, copy_id, [&](stage::CopySsnTable &s, stage::CopySsn &) {
        auto it = s.readers.find(copy_id);
        const uint32_t k = it == s.readers.end() ? 0u : (uint32_t)it->second.size();
        for (uint32_t i = 0; i < k && i < max; ++i) read_ids[i] = it->second[i];
        *count = k;
        return STAGE_OK;
    });
}

// EphemeralPool::OverwriteVersionHeader::AddReader (ephemeral_pool.h:61-65), called by BTree::Read
// for a read served from the copy (b_tree.cpp:2104-2105)
int stage_copy_add_reader(stage_table *t, uint32_t copy_id, uint32_t read_id) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return with_copy(t, copy_id, [&](stage::CopySsnTable &s, stage::CopySsn &) {
        return guarded([&] {
            s.readers[copy_id].push_back(read_id);
            return STAGE_OK;
        });
    });
}

// IncreaseWRCount (+1: AddCount, refused once the header is waiting) / DecreaseWRCount (-1:
// SubCount), ephemeral_pool.cpp:69-103
int stage_copy_wr_count(stage_table *t, uint32_t copy_id, int delta, int *ok) {
    if (!t || !ok || (delta != 1 && delta != -1)) return fail(STAGE_E_ARG, "bad arguments");
    return with_copy(t, copy_id, [&](stage::CopySsnTable &, stage::CopySsn &c) {
        if (delta > 0) {
            *ok = c.waiting ? 0 : 1;
            if (*ok) ++c.count;
        } else {
            --c.count;
            *ok = 1;
        }
        return STAGE_OK;
    });
}

// UpdatePs (ephemeral_pool.cpp:194-205)
int stage_copy_update_ps(stage_table *t, uint32_t copy_id, uint32_t pstamp) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return with_copy(t, copy_id, [&](stage::CopySsnTable &, stage::CopySsn &c) {
        c.pstamp = pstamp;
        return STAGE_OK;
    });
}

int stage_import_leaf_images(stage_table *t, const uint8_t *blocks, uint64_t n_leaves, uint32_t block_size,
                             const uint64_t *sep_keys, const uint16_t *sep_lens, uint64_t *n_records) {
    if (!t || !blocks || (!sep_keys != !sep_lens)) return fail(STAGE_E_ARG, "bad arguments");
    return guarded([&] {
        const uint64_t n = host(t).import_leaf_images(blocks, n_leaves, block_size, sep_keys, sep_lens);
        if (n_records) *n_records = n;
        return STAGE_OK;
    });
}

int stage_probe_batch(stage_table *t, const uint64_t *d_keys, const uint16_t *d_lens, const uint32_t *d_read_ids,
                      const uint32_t *d_leaf_ids, uint64_t n, stage_probe_out *d_out, uint8_t *d_records,
                      void *stream) {
    int rc = need_synced(t);
    if (rc) return rc;
    if (n && (!d_keys || !d_out)) return fail(STAGE_E_ARG, "null device buffer");
    hipError_t e = hipSetDevice(t->dev.device);
    if (e != hipSuccess) return hip_rc(e, "hipSetDevice");
    stage::DevTable view = t->dev.view;
    if (t->out_stride) view.stride = t->out_stride;
    stage::ProbeTuning tune = t->tune;
    tune.status_bytes = t->status_bytes;
    e = stage::launch_probe(view, d_keys, d_lens, d_read_ids, d_leaf_ids, n,
                            reinterpret_cast<stage::stage_probe_out_dev *>(d_out), d_records, pick(t, stream), tune);
    return hip_rc(e, "probe kernel");
}

uint32_t stage_window_stride(uint32_t len) { return (len + 15u) & ~15u; }

int stage_probe_batch_window(stage_table *t, const uint64_t *d_keys, const uint16_t *d_lens, const uint32_t *d_read_ids,
                             const uint32_t *d_leaf_ids, uint64_t n, uint32_t payload_off, uint32_t len,
                             stage_probe_out *d_out, uint8_t *d_window, void *stream) {
    int rc = check_window(t, payload_off, len);
    if (rc) return rc;
    if (n && (!d_keys || !d_out || !d_window)) return fail(STAGE_E_ARG, "null device buffer");
    rc = need_synced(t);
    if (rc) return rc;
    if (n == 0) return STAGE_OK;
    hipError_t e = hipSetDevice(t->dev.device);
    if (e != hipSuccess) return hip_rc(e, "hipSetDevice");
    stage::ProbeTuning tune = t->tune;
    tune.status_bytes = t->status_bytes;
    e = stage::launch_probe_window(t->dev.view, d_keys, d_lens, d_read_ids, d_leaf_ids, n,
                                   facts(t).key_pad() + payload_off, len,
                                   reinterpret_cast<stage::stage_probe_out_dev *>(d_out), d_window, pick(t, stream), tune);
    return hip_rc(e, "window probe kernel");
}

int stage_probe_batch_ex(stage_table *t, const uint64_t *d_keys, const uint16_t *d_lens, const uint32_t *d_read_ids,
                         const uint32_t *d_leaf_ids, const uint8_t *d_for_update, uint64_t n, stage_probe_out *d_out,
                         uint8_t *d_records, void *stream) {
    if (!d_for_update) return stage_probe_batch(t, d_keys, d_lens, d_read_ids, d_leaf_ids, n, d_out, d_records, stream);
    if (!t) return fail(STAGE_E_ARG, "null table");
    if (t->status_bytes != 32)
        return fail(STAGE_E_UNSUPPORTED, "is_for_update probes need the 32-B status records (stage_set_output_layout)");
    int rc = stage_probe_batch(t, d_keys, d_lens, d_read_ids, d_leaf_ids, n, d_out, d_records, stream);
    if (rc) return rc;
    stage::DevTable view = t->dev.view;
    if (t->out_stride) view.stride = t->out_stride;
    return hip_rc(stage::launch_for_update(view, d_for_update, d_read_ids, n,
                                           reinterpret_cast<stage::stage_probe_out_dev *>(d_out), d_records,
                                           pick(t, stream)),
                  "for-update kernel");
}

int stage_set_output_layout(stage_table *t, uint32_t row_stride, uint32_t status_bytes) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    const uint32_t row = (host(t).key_pad() + host(t).params().payload_size + 15) & ~15u;
    if (row_stride && (row_stride < row || row_stride % 16))
        return fail(STAGE_E_ARG, "row_stride: 0 or a multiple of 16 of at least the row bytes (key pad + payload)");
    if (status_bytes != 32 && status_bytes != 16) return fail(STAGE_E_ARG, "status_bytes: 32 or 16");
    if (status_bytes == 16 && (host(t).params().key_width == 0 || host(t).key_words() != 1 || host(t).cap() != 64))
        return fail(STAGE_E_ARG, "16-B status records: fixed-width keys of <= 8 bytes in 64-slot leaves");
    t->out_stride = row_stride;
    t->status_bytes = (int)status_bytes;
    return STAGE_OK;
}

int stage_scan_batch(stage_table *t, const uint64_t *d_start_keys, const uint16_t *d_lens, uint64_t n,
                     uint32_t scan_size, uint32_t *d_counts, uint8_t *d_records, void *stream) {
    int rc = need_synced(t);
    if (rc) return rc;
    if (n && (!d_start_keys || !d_counts || (!d_records && scan_size))) return fail(STAGE_E_ARG, "null device buffer");
    hipError_t e = hipSetDevice(t->dev.device);
    if (e != hipSuccess) return hip_rc(e, "hipSetDevice");
    e = stage::launch_scan(t->dev.view, d_start_keys, d_lens, n, scan_size, d_counts, d_records, pick(t, stream),
                          t->scan_tune);
    return hip_rc(e, "scan kernel");
}

int stage_index_scan_batch(stage_table *t, const uint64_t *d_start_keys, const uint16_t *d_lens,
                           const uint32_t *d_read_ids, uint64_t n, uint32_t scan_size, uint32_t *d_counts,
                           uint8_t *d_records, uint8_t *d_row_status, void *stream) {
    int rc = need_synced(t);
    if (rc) return rc;
    if (n && (!d_start_keys || !d_counts || (scan_size && (!d_records || !d_row_status))))
        return fail(STAGE_E_ARG, "null device buffer");
    hipError_t e = hipSetDevice(t->dev.device);
    if (e != hipSuccess) return hip_rc(e, "hipSetDevice");
    e = stage::launch_scan(t->dev.view, d_start_keys, d_lens, n, scan_size, d_counts, d_records, pick(t, stream),
                           t->scan_tune, d_read_ids, d_row_status);
    return hip_rc(e, "index scan kernel");
}

// both window scans: d_row_status non-null selects the index-scan form
static int scan_window(stage_table *t, const uint64_t *d_start_keys, const uint16_t *d_lens, const uint32_t *d_read_ids,
                       uint64_t n, uint32_t scan_size, uint32_t payload_off, uint32_t len, uint32_t *d_counts,
                       uint8_t *d_window, uint8_t *d_row_keys, uint8_t *d_row_status, bool index, void *stream) {
    int rc = check_window(t, payload_off, len);
    if (rc) return rc;
    if (n && scan_size && (!d_start_keys || !d_counts || !d_window || (index && !d_row_status)))
        return fail(STAGE_E_ARG, "null device buffer");
    rc = need_synced(t);
    if (rc) return rc;
    if (n == 0) return STAGE_OK;
    hipError_t e = hipSetDevice(t->dev.device);
    if (e != hipSuccess) return hip_rc(e, "hipSetDevice");
    e = stage::launch_scan_window(t->dev.view, d_start_keys, d_lens, n, scan_size, facts(t).key_pad() + payload_off, len,
                                  facts(t).key_pad(), d_counts, d_window, d_row_keys, pick(t, stream), t->scan_tune,
                                  index ? d_read_ids : nullptr, index ? d_row_status : nullptr);
    return hip_rc(e, index ? "window index scan kernel" : "window scan kernel");
}

int stage_scan_batch_window(stage_table *t, const uint64_t *d_start_keys, const uint16_t *d_lens, uint64_t n,
                            uint32_t scan_size, uint32_t payload_off, uint32_t len, uint32_t *d_counts,
                            uint8_t *d_window, uint8_t *d_row_keys, void *stream) {
    return scan_window(t, d_start_keys, d_lens, nullptr, n, scan_size, payload_off, len, d_counts, d_window, d_row_keys,
                       nullptr, false, stream);
}

int stage_index_scan_batch_window(stage_table *t, const uint64_t *d_start_keys, const uint16_t *d_lens,
                                  const uint32_t *d_read_ids, uint64_t n, uint32_t scan_size, uint32_t payload_off,
                                  uint32_t len, uint32_t *d_counts, uint8_t *d_window, uint8_t *d_row_keys,
                                  uint8_t *d_row_status, void *stream) {
    return scan_window(t, d_start_keys, d_lens, d_read_ids, n, scan_size, payload_off, len, d_counts, d_window,
                       d_row_keys, d_row_status, true, stream);
}

static_assert(sizeof(stage_scan_pred) == 24 && sizeof(stage_scan_agg) == 32, "stage_hip.h layout");
static_assert(sizeof(stage_scan_group) == 24, "stage_hip.h layout");
static_assert(STAGE_PRED_MAX == stage::kScanPredMax, "stage_hip.h mirrors kernel_api.hpp");
static_assert(STAGE_GROUP_MAX == stage::kGroupMax && STAGE_GROUP_LDS_MAX == stage::kGroupLdsMax,
              "stage_hip.h mirrors kernel_api.hpp");

// one integer column (payload_off, width) against the table's parameters alone; in_key: the
// column is a field of the row's key, `payload_off` a byte of the row's first key_pad bytes
static int check_column(stage_table *t, const char *what, uint32_t payload_off, uint32_t width, bool in_key = false) {
    if (!stage::scan_column_width(width)) return fail(STAGE_E_ARG, std::string(what) + ": width must be 1, 2, 4 or 8");
    if (in_key && (uint64_t)payload_off + width > facts(t).key_pad())
        return fail(STAGE_E_ARG, std::string(what) + ": off + width exceeds the table's padded key");
    if (!in_key && (uint64_t)payload_off + width > facts(t).params().payload_size)
        return fail(STAGE_E_ARG, std::string(what) + ": payload_off + width exceeds the table's payload_size");
    return STAGE_OK;
}

// the predicates of a filtered scan, checked without a device image and turned into row-byte form
static int check_preds(stage_table *t, const stage_scan_pred *preds, uint32_t n_pred, stage::ScanPreds &out) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    if (n_pred > STAGE_PRED_MAX) return fail(STAGE_E_ARG, "predicates: n_pred exceeds STAGE_PRED_MAX");
    if (n_pred && !preds) return fail(STAGE_E_ARG, "predicates: null preds with n_pred != 0");
    out = stage::ScanPreds{};
    out.n = n_pred;
    for (uint32_t k = 0; k < n_pred; ++k) {
        const stage_scan_pred &p = preds[k];
        int rc = check_column(t, "predicate", p.payload_off, p.width);
        if (rc) return rc;
        if (p.is_signed > 1 || p.negate > 1) return fail(STAGE_E_ARG, "predicate: is_signed and negate are 0 or 1");
        if (p.pad != 0) return fail(STAGE_E_ARG, "predicate: pad must be 0");
        out.p[k] = stage::ScanPred{facts(t).key_pad() + p.payload_off, p.width, p.is_signed, p.negate, 0, p.lo, p.hi};
    }
    return STAGE_OK;
}

// the leaf range of a table scan against the published image (after need_synced)
static int resolve_leaf_range(stage_table *t, uint64_t leaf_begin, uint64_t &leaf_end) {
    const uint64_t nleaves = t->dev.view.nleaves;
    if (leaf_end == UINT64_MAX) leaf_end = nleaves;
    if (leaf_end > nleaves || leaf_begin > leaf_end)
        return fail(STAGE_E_ARG, "table scan: the leaf range exceeds the table's " + std::to_string(nleaves) + " leaves");
    return STAGE_OK;
}

// What a whole-table scan entry point asks for besides the leaf range and the read id.
struct TableScanWindow {  // the window form's payload bytes
    uint32_t payload_off, len;
};
struct TableScanAggColumn {  // the aggregate's column; width 0: the count alone
    uint32_t payload_off, width, is_signed;
};
struct TableScanRequest {
    bool filtered;                  // the _where forms and the aggregate: preds / n_pred are checked
    const stage_scan_pred *preds;
    uint32_t n_pred;
    const TableScanAggColumn *agg;  // null: the scan delivers records
    bool grouped;                   // the grouped aggregate: group is checked
    const stage_scan_group *group;
    const TableScanWindow *window;  // null: rows
    const void *d_result;           // d_count, or d_agg with an aggregate column
    uint64_t max_records;           // records: a record buffer must come with max_records != 0
    const void *d_out;
    const char *kernels;            // names the launch in a HIP error
};
// launch(first leaf, leaves, snapshot mode, read id, the predicates in row-byte form)
using TableScanLaunch = std::function<hipError_t(uint32_t, uint32_t, bool, uint32_t, const stage::ScanPreds &)>;

// Every whole-table scan entry point (TableScanExecutor, executor.h:573-642; per record
// IndexScanExecutor's rule, executor.h:465-534; the per-tuple predicate of executor.h:346-361):
// the argument checks in one order -- predicates, group column, aggregate column, window, leaf
// range, result word, record buffer -- then, on the published image and the table's device, the
// launch.
static int table_scan_call(stage_table *t, uint64_t leaf_begin, uint64_t leaf_end, const uint32_t *read_id,
                           const TableScanRequest &q, const TableScanLaunch &launch) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    stage::ScanPreds p{};
    int rc = q.filtered ? check_preds(t, q.preds, q.n_pred, p) : STAGE_OK;
    if (rc) return rc;
    if (q.grouped) {
        const stage_scan_group *g = q.group;
        if (!g) return fail(STAGE_E_ARG, "group column: null group");
        if (g->is_signed > 1 || g->in_key > 1) return fail(STAGE_E_ARG, "group column: is_signed and in_key are 0 or 1");
        if (g->pad != 0 || g->pad2 != 0) return fail(STAGE_E_ARG, "group column: pad and pad2 must be 0");
        rc = check_column(t, "group column", g->off, g->width, g->in_key != 0);
        if (rc) return rc;
        if (g->n_groups == 0 || g->n_groups > STAGE_GROUP_MAX)
            return fail(STAGE_E_ARG, "group column: n_groups must be 1 .. STAGE_GROUP_MAX");
    }
    rc = q.agg && q.agg->width ? check_column(t, "aggregate column", q.agg->payload_off, q.agg->width) : STAGE_OK;
    if (rc) return rc;
    if (q.agg && q.agg->is_signed > 1) return fail(STAGE_E_ARG, "aggregate column: agg_signed is 0 or 1");
    rc = q.window ? check_window(t, q.window->payload_off, q.window->len) : STAGE_OK;
    if (rc) return rc;
    if (leaf_begin > leaf_end) return fail(STAGE_E_ARG, "table scan: leaf_begin exceeds leaf_end");
    if (!q.d_result)
        return fail(STAGE_E_ARG, q.grouped ? "table scan: null d_groups" : q.agg ? "table scan: null d_agg"
                                                                                  : "table scan: null d_count");
    if (q.max_records && !q.d_out) return fail(STAGE_E_ARG, "table scan: null record buffer with max_records != 0");
    rc = need_synced(t);
    if (rc) return rc;
    rc = resolve_leaf_range(t, leaf_begin, leaf_end);
    if (rc) return rc;
    return guarded([&] {
        hipError_t e = hipSetDevice(t->dev.device);
        if (e != hipSuccess) return hip_rc(e, "hipSetDevice");
        e = launch((uint32_t)leaf_begin, (uint32_t)(leaf_end - leaf_begin), read_id != nullptr, read_id ? *read_id : 0u, p);
        return hip_rc(e, q.kernels);
    });
}

// the four scans that deliver records: `filtered` selects the _where forms, a window the window
// forms, d_out is d_records / d_window
static int table_scan(stage_table *t, uint64_t leaf_begin, uint64_t leaf_end, const uint32_t *read_id, bool filtered,
                      const stage_scan_pred *preds, uint32_t n_pred, const TableScanWindow *window,
                      uint64_t max_records, uint64_t *d_count, uint64_t *d_leaf_offsets, uint8_t *d_out,
                      uint8_t *d_row_keys, uint64_t *d_row_slot, uint64_t *d_row_meta, uint8_t *d_row_status,
                      void *stream) {
    const TableScanRequest q{filtered, preds, n_pred, nullptr, false, nullptr, window, d_count, max_records, d_out,
                             filtered ? "filtered table scan kernels" : "table scan kernels"};
    return table_scan_call(t, leaf_begin, leaf_end, read_id, q,
                           [&](uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid, const stage::ScanPreds &p) {
        const uint64_t bytes = filtered ? stage::table_scan_where_scratch_bytes(nl, t->dev.view.cap)
                                        : stage::table_scan_scratch_bytes(nl);
        uint8_t *scratch = nl ? stage::scratch_bytes(t->dev, bytes) : nullptr;
        const stage::TableScanOut o{max_records, d_count, d_leaf_offsets, window ? nullptr : d_out,
                                    window ? d_out : nullptr, window ? d_row_keys : nullptr, d_row_meta, d_row_status};
        const uint32_t kp = facts(t).key_pad(), row_off = window ? kp + window->payload_off : 0u;
        const uint32_t len = window ? window->len : 0u;
        return filtered ? stage::launch_table_scan_where(t->dev.view, leaf0, nl, snapshot, rid, p, row_off, len, kp, o,
                                                         d_row_slot, scratch, pick(t, stream), t->scan_tune)
                        : stage::launch_table_scan(t->dev.view, leaf0, nl, snapshot, rid, row_off, len, kp, o, scratch,
                                                   pick(t, stream), t->scan_tune);
    });
}

int stage_table_scan(stage_table *t, uint64_t leaf_begin, uint64_t leaf_end, const uint32_t *read_id,
                     uint64_t max_records, uint64_t *d_count, uint64_t *d_leaf_offsets, uint8_t *d_records,
                     uint64_t *d_row_meta, uint8_t *d_row_status, void *stream) {
    return table_scan(t, leaf_begin, leaf_end, read_id, false, nullptr, 0, nullptr, max_records, d_count, d_leaf_offsets,
                      d_records, nullptr, nullptr, d_row_meta, d_row_status, stream);
}

int stage_table_scan_window(stage_table *t, uint64_t leaf_begin, uint64_t leaf_end, const uint32_t *read_id,
                            uint32_t payload_off, uint32_t len, uint64_t max_records, uint64_t *d_count,
                            uint64_t *d_leaf_offsets, uint8_t *d_window, uint8_t *d_row_keys, uint64_t *d_row_meta,
                            uint8_t *d_row_status, void *stream) {
    const TableScanWindow w{payload_off, len};
    return table_scan(t, leaf_begin, leaf_end, read_id, false, nullptr, 0, &w, max_records, d_count, d_leaf_offsets,
                      d_window, d_row_keys, nullptr, d_row_meta, d_row_status, stream);
}

int stage_table_scan_where(stage_table *t, uint64_t leaf_begin, uint64_t leaf_end, const uint32_t *read_id,
                           const stage_scan_pred *preds, uint32_t n_pred, uint64_t max_records, uint64_t *d_count,
                           uint64_t *d_leaf_offsets, uint8_t *d_records, uint64_t *d_row_slot, uint64_t *d_row_meta,
                           uint8_t *d_row_status, void *stream) {
    return table_scan(t, leaf_begin, leaf_end, read_id, true, preds, n_pred, nullptr, max_records, d_count,
                      d_leaf_offsets, d_records, nullptr, d_row_slot, d_row_meta, d_row_status, stream);
}

int stage_table_scan_where_window(stage_table *t, uint64_t leaf_begin, uint64_t leaf_end, const uint32_t *read_id,
                                  const stage_scan_pred *preds, uint32_t n_pred, uint32_t payload_off, uint32_t len,
                                  uint64_t max_records, uint64_t *d_count, uint64_t *d_leaf_offsets, uint8_t *d_window,
                                  uint8_t *d_row_keys, uint64_t *d_row_slot, uint64_t *d_row_meta,
                                  uint8_t *d_row_status, void *stream) {
    const TableScanWindow w{payload_off, len};
    return table_scan(t, leaf_begin, leaf_end, read_id, true, preds, n_pred, &w, max_records, d_count, d_leaf_offsets,
                      d_window, d_row_keys, d_row_slot, d_row_meta, d_row_status, stream);
}

int stage_table_scan_aggregate(stage_table *t, uint64_t leaf_begin, uint64_t leaf_end, const uint32_t *read_id,
                               const stage_scan_pred *preds, uint32_t n_pred, uint32_t agg_off, uint32_t agg_width,
                               uint32_t agg_signed, stage_scan_agg *d_agg, void *stream) {
    const TableScanAggColumn col{agg_off, agg_width, agg_signed};
    const TableScanRequest q{true, preds, n_pred, &col, false, nullptr, nullptr, d_agg, 0, nullptr,
                             "table scan aggregate kernels"};
    return table_scan_call(t, leaf_begin, leaf_end, read_id, q,
                           [&](uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid, const stage::ScanPreds &p) {
        const uint64_t bytes = stage::table_scan_aggregate_scratch_bytes(nl, t->scan_tune);
        uint8_t *scratch = nl ? stage::scratch_bytes(t->dev, bytes) : nullptr;
        return stage::launch_table_scan_aggregate(t->dev.view, leaf0, nl, snapshot, rid, p, facts(t).key_pad() + agg_off,
                                                  agg_width, agg_signed != 0, reinterpret_cast<uint64_t *>(d_agg), scratch,
                                                  pick(t, stream), t->scan_tune);
    });
}

int stage_table_scan_group_aggregate(stage_table *t, uint64_t leaf_begin, uint64_t leaf_end, const uint32_t *read_id,
                                     const stage_scan_pred *preds, uint32_t n_pred, const stage_scan_group *group,
                                     uint32_t agg_off, uint32_t agg_width, uint32_t agg_signed, stage_scan_agg *d_groups,
                                     void *stream) {
    const TableScanAggColumn col{agg_off, agg_width, agg_signed};
    const TableScanRequest q{true, preds, n_pred, &col, true, group, nullptr, d_groups, 0, nullptr,
                             "table scan group aggregate kernels"};
    return table_scan_call(t, leaf_begin, leaf_end, read_id, q,
                           [&](uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid, const stage::ScanPreds &p) {
        const uint32_t kp = facts(t).key_pad();
        const stage::ScanGroupSpec g{group->in_key ? group->off : kp + group->off, group->width, group->is_signed != 0,
                                     (uint64_t)group->base, group->n_groups};
        const uint64_t bytes = stage::table_scan_group_scratch_bytes(nl, g.n, t->scan_tune, t->group_tune);
        uint8_t *scratch = bytes ? stage::scratch_bytes(t->dev, bytes) : nullptr;
        return stage::launch_table_scan_group(t->dev.view, leaf0, nl, snapshot, rid, p, g, kp + agg_off, agg_width,
                                              agg_signed != 0, reinterpret_cast<uint64_t *>(d_groups), scratch,
                                              pick(t, stream), t->scan_tune, t->group_tune);
    });
}

int stage_index_scan_first_batch(stage_table *t, const uint64_t *d_start_keys, const uint32_t *d_read_ids,
                                 uint64_t n, uint32_t scan_size, uint32_t prefix_words, uint32_t *d_image,
                                 uint8_t *d_status, void *stream) {
    int rc = need_synced(t);
    if (rc) return rc;
    if (t->dev.view.key_width == 0) return fail(STAGE_E_ARG, "first-tuple scans need fixed-width keys");
    if (scan_size == 0 || scan_size > 63) return fail(STAGE_E_ARG, "scan_size must be 1..63");
    if (prefix_words > t->dev.view.key_words) return fail(STAGE_E_ARG, "prefix_words exceeds the key's words");
    if (n && (!d_start_keys || !d_image || !d_status)) return fail(STAGE_E_ARG, "null device buffer");
    hipError_t e = hipSetDevice(t->dev.device);
    if (e != hipSuccess) return hip_rc(e, "hipSetDevice");
    e = stage::launch_scan_first(t->dev.view, d_start_keys, n, scan_size, d_read_ids, prefix_words, d_image, d_status,
                                 pick(t, stream), t->scan_tune);
    return hip_rc(e, "first-tuple scan kernel");
}

int stage_resolve_batch(stage_table *t, const uint64_t *d_keys, const uint16_t *d_lens, uint64_t n, int le_child,
                        uint32_t *d_leaf, void *stream) {
    int rc = need_synced(t);
    if (rc) return rc;
    if (n && (!d_keys || !d_leaf)) return fail(STAGE_E_ARG, "null device buffer");
    hipError_t e = hipSetDevice(t->dev.device);
    if (e != hipSuccess) return hip_rc(e, "hipSetDevice");
    e = stage::launch_resolve(t->dev.view, d_keys, d_lens, n, le_child, d_leaf, pick(t, stream));
    return hip_rc(e, "resolve kernel");
}

int stage_set_probe_tuning(stage_table *t, int group, int max_blocks) {
    if (!t || (group != 1 && group != 2 && group != 4 && group != 8) || max_blocks < 0)
        return fail(STAGE_E_ARG, "bad tuning");
    t->tune.group = group;
    t->tune.max_blocks = max_blocks;
    return STAGE_OK;
}

int stage_set_scan_tuning(stage_table *t, int max_blocks) {
    if (!t || max_blocks < 0) return fail(STAGE_E_ARG, "bad tuning");
    t->scan_tune.max_blocks = max_blocks;
    return STAGE_OK;
}

int stage_set_scan_group_tuning(stage_table *t, int lds_max, int combine) {
    if (!t || lds_max < -1 || lds_max > (int)STAGE_GROUP_LDS_MAX || combine < -1 || combine > 64)
        return fail(STAGE_E_ARG, "bad tuning");
    t->group_tune.lds_max = lds_max;
    t->group_tune.combine = combine;
    return STAGE_OK;
}

int stage_set_probe_store(stage_table *t, int policy) {
    if (!t || policy < STAGE_STORE_TEMPORAL || policy > STAGE_STORE_WRITE_THROUGH)
        return fail(STAGE_E_ARG, "bad store policy");
    t->tune.store = policy;
    return STAGE_OK;
}

int stage_set_probe_form(stage_table *t, int form) {
    if (!t || (form != STAGE_PROBE_FORM_WAVE && form != STAGE_PROBE_FORM_LANE))
        return fail(STAGE_E_ARG, "bad probe form");
    t->tune.form = form;
    return STAGE_OK;
}

int stage_murmur64a_batch(const void *d_keys, uint32_t key_len, uint32_t key_stride, uint64_t seed, uint64_t n,
                          uint64_t *d_out, void *stream) {
    if (n && (!d_keys || !d_out || key_stride < key_len)) return fail(STAGE_E_ARG, "bad arguments");
    return hip_rc(stage::launch_murmur(d_keys, key_len, key_stride, seed, n, d_out, (hipStream_t)stream),
                  "murmur kernel");
}

// ---- plumbing
int stage_set_device(int device) { return hip_rc(hipSetDevice(device), "hipSetDevice"); }
int stage_device_count(int *count) { return hip_rc(hipGetDeviceCount(count), "hipGetDeviceCount"); }
int stage_dev_alloc(uint64_t bytes, void **ptr) { return hip_rc(hipMalloc(ptr, bytes ? bytes : 16), "hipMalloc"); }
int stage_dev_free(void *ptr) { return hip_rc(hipFree(ptr), "hipFree"); }
int stage_dev_memset(void *ptr, int value, uint64_t bytes, void *stream) {
    return hip_rc(hipMemsetAsync(ptr, value, bytes, (hipStream_t)stream), "hipMemsetAsync");
}
int stage_memcpy_h2d(void *dst, const void *src, uint64_t bytes, void *stream) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return hip_rc(e, "h2d");
}
int stage_memcpy_d2h(void *dst, const void *src, uint64_t bytes, void *stream) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return hip_rc(e, "d2h");
}
int stage_stream_create(void **stream) {
    return hip_rc(hipStreamCreateWithFlags((hipStream_t *)stream, hipStreamNonBlocking), "hipStreamCreate");
}
int stage_stream_destroy(void *stream) { return hip_rc(hipStreamDestroy((hipStream_t)stream), "hipStreamDestroy"); }
int stage_stream_sync(void *stream) { return hip_rc(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize"); }
int stage_device_sync(void) { return hip_rc(hipDeviceSynchronize(), "hipDeviceSynchronize"); }
int stage_event_create(void **ev) { return hip_rc(hipEventCreate((hipEvent_t *)ev), "hipEventCreate"); }
int stage_event_destroy(void *ev) { return hip_rc(hipEventDestroy((hipEvent_t)ev), "hipEventDestroy"); }
int stage_event_record(void *ev, void *stream) {
    return hip_rc(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream), "hipEventRecord");
}
int stage_event_elapsed(void *a, void *b, float *ms) {
    hipError_t e = hipEventSynchronize((hipEvent_t)b);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b);
    return hip_rc(e, "hipEventElapsedTime");
}

// ---- multi-GPU
int stage_comm_unique_id(uint8_t *id128) {
    if (!id128) return fail(STAGE_E_ARG, "null argument");
    return guarded([&] { return stage::shard_unique_id(id128); });
}

int stage_comm_init(stage_table *t, const uint8_t *id128, int rank, int world) {
    if (!t || !id128 || world < 1 || rank < 0 || rank >= world) return fail(STAGE_E_ARG, "bad arguments");
    if (facts(t).key_words() != 1) return fail(STAGE_E_ARG, "the sharded front-end routes keys of <= 8 bytes");
    return guarded([&] {
        (void)hipSetDevice(t->dev.device);
        t->comm = std::make_unique<stage::ShardComm>();
        const int rc = stage::shard_init(*t->comm, id128, rank, world, t->shard_chunks);
        if (t->shard_dedupe >= 0) t->comm->dedupe = t->shard_dedupe != 0;
        t->comm->key_bits = t->shard_key_bits;
        return rc;
    });
}

int stage_set_shard_dedupe(stage_table *t, int on) {
    if (!t || on < -1 || on > 1) return fail(STAGE_E_ARG, "dedupe must be -1, 0 or 1");
    t->shard_dedupe = on;
    const bool v = on < 0 ? stage::shard_default_dedupe() : on != 0;
    if (t->comm) t->comm->dedupe = v;
    if (t->loop_comm) t->loop_comm->dedupe = v;
    return STAGE_OK;
}

int stage_set_write_overlap(stage_table *t, int on) {
    if (!t || on < 0 || on > 1) return fail(STAGE_E_ARG, "write overlap must be 0 or 1");
    t->wp_overlap = on;
    return STAGE_OK;
}

int stage_set_shard_key_bits(stage_table *t, int bits) {
    if (!t || bits < 0 || bits > 64) return fail(STAGE_E_ARG, "bits must be 0..64");
    t->shard_key_bits = bits ? bits : 64;
    if (t->comm) t->comm->key_bits = t->shard_key_bits;
    if (t->loop_comm) t->loop_comm->key_bits = t->shard_key_bits;
    return STAGE_OK;
}

int stage_rccl_info(int *runtime_version, int *header_version, char *path, uint64_t path_len) {
    return guarded([&] { return stage::shard_rccl_info(runtime_version, header_version, path, path_len); });
}

int stage_sharded_stats(stage_table *t, int loopback, uint64_t *n_keys, uint64_t *n_routed, uint64_t *n_remote) {
    if (!t || !n_keys || !n_routed || !n_remote) return fail(STAGE_E_ARG, "null argument");
    stage::ShardComm *c = loopback ? t->loop_comm.get() : t->comm.get();
    if (!c) return fail(STAGE_E_STATE, "no sharded probe has run");
    *n_keys = c->last_n;
    *n_routed = c->last_routed;
    *n_remote = c->last_remote;
    return STAGE_OK;
}

int stage_sharded_stats_ex(stage_table *t, int loopback, uint64_t *v, int nv) {
    if (!t || !v || nv < 0) return fail(STAGE_E_ARG, "bad arguments");
    stage::ShardComm *c = loopback ? t->loop_comm.get() : t->comm.get();
    if (!c) return fail(STAGE_E_STATE, "no sharded probe has run");
    const uint64_t all[4] = {c->last_n, c->last_routed, c->last_remote, c->last_received};
    for (int i = 0; i < nv && i < 4; ++i) v[i] = all[i];
    return STAGE_OK;
}

int stage_comm_allreduce_f64(stage_table *t, double *values, uint64_t n, int op) {
    if (!t || (!values && n) || op < 0 || op > 2) return fail(STAGE_E_ARG, "bad arguments");
    if (!t->comm) return fail(STAGE_E_STATE, "stage_comm_init first");
    return guarded([&] {
        (void)hipSetDevice(t->dev.device);
        return stage::shard_allreduce_f64(*t->comm, values, n, op);
    });
}

int stage_comm_allgather_f64(stage_table *t, const double *in, uint64_t n, double *out) {
    if (!t || ((!in || !out) && n)) return fail(STAGE_E_ARG, "bad arguments");
    if (!t->comm) return fail(STAGE_E_STATE, "stage_comm_init first");
    return guarded([&] {
        (void)hipSetDevice(t->dev.device);
        return stage::shard_allgather_f64(*t->comm, in, n, out);
    });
}

int stage_set_shard_chunks(stage_table *t, int chunks) {
    if (!t || chunks < 0 || chunks > 64) return fail(STAGE_E_ARG, "chunks must be 0..64");
    t->shard_chunks = chunks;
    return STAGE_OK;
}

int stage_comm_destroy(stage_table *t) {
    if (!t) return fail(STAGE_E_ARG, "null table");
    return guarded([&] {
        t->comm.reset();
        return STAGE_OK;
    });
}

int stage_probe_sharded(stage_table *t, const uint64_t *d_keys, const uint32_t *d_read_ids, uint64_t n,
                        stage_probe_out *d_out, uint8_t *d_records, void *stream) {
    int rc = need_synced(t);
    if (rc) return rc;
    if (!t->comm) return fail(STAGE_E_STATE, "stage_comm_init first");
    return guarded([&] {
        (void)hipSetDevice(t->dev.device);
        // the caller's row stride (stage_set_output_layout) is also the stride the rows travel
        // at: one row layout from the owner's probe to the caller's position
        stage::DevTable view = t->dev.view;
        if (t->out_stride) view.stride = t->out_stride;
        return stage::shard_probe(*t->comm, view, t->tune, d_keys, d_read_ids, n,
                                  reinterpret_cast<stage::stage_probe_out_dev *>(d_out), d_records, STAGE_REPLY_ROWS,
                                  pick(t, stream));
    });
}

int stage_probe_sharded_ex(stage_table *t, const uint64_t *d_keys, const uint32_t *d_read_ids, uint64_t n,
                           stage_probe_out *d_out, uint8_t *d_records, int reply_mode, void *stream) {
    int rc = need_synced(t);
    if (rc) return rc;
    if (!t->comm) return fail(STAGE_E_STATE, "stage_comm_init first");
    if (reply_mode != STAGE_REPLY_ROWS && reply_mode != STAGE_REPLY_OWNER && reply_mode != STAGE_REPLY_PEER &&
        reply_mode != STAGE_REPLY_DIRECT)
        return fail(STAGE_E_ARG, "bad reply mode");
    return guarded([&] {
        (void)hipSetDevice(t->dev.device);
        // the caller's row stride (stage_set_output_layout) is also the stride the rows travel
        // at: one row layout from the owner's probe to the caller's position
        stage::DevTable view = t->dev.view;
        if (t->out_stride) view.stride = t->out_stride;
        return stage::shard_probe(*t->comm, view, t->tune, d_keys, d_read_ids, n,
                                  reinterpret_cast<stage::stage_probe_out_dev *>(d_out), d_records, reply_mode,
                                  pick(t, stream));
    });
}

int stage_sharded_owner_rows(stage_table *t, int loopback, uint8_t **d_rows, uint64_t *n_rows) {
    if (!t || !d_rows || !n_rows) return fail(STAGE_E_ARG, "null argument");
    stage::ShardComm *c = loopback ? t->loop_comm.get() : t->comm.get();
    if (!c) return fail(STAGE_E_STATE, "no sharded probe has run");
    *d_rows = (uint8_t *)c->rrec;
    *n_rows = c->owner_rows;
    return STAGE_OK;
}

int stage_probe_sharded_loopback(stage_table *const *shards, int world, const uint64_t *const *d_keys,
                                 const uint32_t *const *d_read_ids, const uint64_t *n, stage_probe_out *const *d_out,
                                 uint8_t *const *d_records, int reply_mode, void *stream) {
    if (!shards || world < 1 || !d_keys || !n || !d_out || !d_records) return fail(STAGE_E_ARG, "null argument");
    if (reply_mode != STAGE_REPLY_ROWS && reply_mode != STAGE_REPLY_OWNER && reply_mode != STAGE_REPLY_PEER &&
        reply_mode != STAGE_REPLY_DIRECT)
        return fail(STAGE_E_ARG, "bad reply mode");
    for (int r = 0; r < world; ++r) {
        int rc = need_synced(shards[r]);
        if (rc) return rc;
        if (facts(shards[r]).key_words() != 1) return fail(STAGE_E_ARG, "the sharded front-end routes keys of <= 8 bytes");
        if (shards[r]->dev.device != shards[0]->dev.device) return fail(STAGE_E_ARG, "shards on different devices");
        if ((d_records[r] == nullptr) != (d_records[0] == nullptr)) return fail(STAGE_E_ARG, "rows for all or none");
    }
    return guarded([&] {
        (void)hipSetDevice(shards[0]->dev.device);
        std::vector<stage::ShardComm *> cs(world);
        std::vector<const stage::DevTable *> ts(world);
        std::vector<stage::DevTable> views(world);
        std::vector<const uint64_t *> ks(world);
        std::vector<const uint32_t *> rs(world);
        std::vector<uint64_t> ns(world);
        std::vector<stage::stage_probe_out_dev *> os(world);
        std::vector<uint8_t *> recs(world);
        for (int r = 0; r < world; ++r) {
            stage_table *t = shards[r];
            const int want = shards[0]->shard_chunks > 0 ? shards[0]->shard_chunks : stage::shard_default_chunks(world);
            if (!t->loop_comm || t->loop_comm->world != world || t->loop_comm->rank != r ||
                t->loop_comm->chunks != want) {
                t->loop_comm = std::make_unique<stage::ShardComm>();
                stage::shard_init_loopback(*t->loop_comm, r, world, want);
            }
            if (t->shard_dedupe >= 0) t->loop_comm->dedupe = t->shard_dedupe != 0;
            t->loop_comm->key_bits = t->shard_key_bits;
            cs[r] = t->loop_comm.get();
            views[r] = t->dev.view;
            if (shards[0]->out_stride) views[r].stride = shards[0]->out_stride;  // as stage_probe_sharded_ex
            ts[r] = &views[r];
            ks[r] = d_keys[r];
            rs[r] = d_read_ids ? d_read_ids[r] : nullptr;
            ns[r] = n[r];
            os[r] = reinterpret_cast<stage::stage_probe_out_dev *>(d_out[r]);
            recs[r] = d_records[r];
        }
        return stage::shard_probe_loopback(cs, ts, shards[0]->tune, ks, rs, ns, os, recs, reply_mode,
                                           pick(shards[0], stream));
    });
}

}  // extern "C"

namespace stage {
void set_error(const std::string &msg) { g_err = msg; }
}  // namespace stage
