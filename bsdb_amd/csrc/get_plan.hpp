// get_plan.hpp -- what the batched reader (capi_get.hip, get_kernels.hip)
// allocates and launches, decided on the host from plain numbers: the layout
// of the resident kv.db image (get_layout), whether an open fits the free
// memory (get_open_fits), how the host forms cut their queries into chunks
// (get_host_chunk), the grid of the locate launch (the gather's is
// piece_grid, piece_plan.hpp), and the address decode with its bounds test
// (get_decode), which the locate kernel calls too.  C++17 without HIP or getenv, so the arithmetic runs (and is
// checked, tests/get_plan_check.cpp) without a GPU.
//   read/SyncReader.java:44-57, read/kv/PartitionedKVReader.java:78-82,
//   read/kv/BlockedKVReader.java:42-52, read/kv/BaseKVReader.java:16-31
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "piece_plan.hpp"  // the gather's grid (piece_grid); BSDB_HD

namespace bsdb {

constexpr int GET_MAX_PARTS = 128;                // addr >>> 56 of a non-negative address
constexpr uint64_t GET_MAX_FILE = 1ull << 56;     // a partition file's offsets are 56 bits
constexpr uint64_t GET_PAGE = 4096;               // NativeFileIO.PAGE_SIZE
constexpr uint64_t GET_GRID_MAX = 0xFFFFFFFFull;  // a launch's workgroups stay below 2^32
constexpr uint64_t GET_DEFAULT_BATCH = 1ull << 22;
constexpr uint64_t GET_BATCH_KEY_BYTES = 256ull << 20;  // key bytes of one host chunk, at most
constexpr uint64_t GET_RESERVE = 256ull << 20;          // left free by an open: the host forms' chunk buffers

enum GetStatus { GET_FOUND = 0, GET_REJECTED = 1, GET_KEY_MISMATCH = 2, GET_BAD_ADDR = 3 };
enum GetWord { GW_QUERIES = 0, GW_FOUND, GW_REJECTED, GW_KEY_MISMATCH, GW_BAD_ADDR, GW_VALUE_BYTES, GW_WORDS };

// The image: every partition file at a 16-byte aligned base of one allocation.
struct GetLayout {
    bool ok = false;  // false: a count or a size out of range
    int partitions = 0;
    uint64_t base[GET_MAX_PARTS] = {};
    uint64_t total = 0;  // bytes of the allocation (the last partition's end, rounded up to 16)
};

inline GetLayout get_layout(const uint64_t *sizes, int partitions) {
    GetLayout l;
    if (partitions < 1 || partitions > GET_MAX_PARTS) return l;
    uint64_t end = 0;  // <= 128 * 2^56 = 2^63: nothing wraps
    for (int p = 0; p < partitions; ++p) {
        if (sizes[p] > GET_MAX_FILE) return l;
        l.base[p] = end;
        end = (end + sizes[p] + 15) & ~15ull;
    }
    l.partitions = partitions;
    l.total = end;
    l.ok = true;
    return l;
}

// device bytes an open allocates: the image and index.db (exact), or
// index_a.db alone (approximate); plus the partition table and the report
inline uint64_t get_open_bytes(uint64_t image_bytes, uint64_t n, bool approximate) {
    return (approximate ? 0 : image_bytes) + 8 * n + 2 * 8 * (uint64_t)GET_MAX_PARTS + 64;
}

inline bool get_open_fits(uint64_t image_bytes, uint64_t n, bool approximate, uint64_t free_bytes) {
    if (n > (1ull << 58) || image_bytes > (1ull << 63)) return false;
    const uint64_t need = get_open_bytes(image_bytes, n, approximate);
    return free_bytes >= GET_RESERVE && need <= free_bytes - GET_RESERVE;
}

// queries of one chunk of a host form: the caller's batch (0 = default), cut
// so that a chunk of fixed-length keys stays under GET_BATCH_KEY_BYTES
// (key_len 0: variable length, cut by the key bytes where the chunk is made)
inline uint64_t get_host_chunk(uint64_t batch, uint32_t key_len) {
    uint64_t c = batch ? batch : GET_DEFAULT_BATCH;
    if (key_len) c = std::min<uint64_t>(c, std::max<uint64_t>(1, GET_BATCH_KEY_BYTES / key_len));
    return std::max<uint64_t>(1, c);
}

// k_get_locate: a query per lane, grid-stride
inline uint32_t get_locate_grid(uint64_t nq, int num_cus) {
    const uint64_t cus = (uint64_t)std::max(1, num_cus);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(nq >> 8) + ((nq & 255) != 0), cus * 16, GET_GRID_MAX}));
}

// Where an address says its record is.  ok: the 3-byte header [pos, pos + 3)
// lies below `limit`, both offsets into partition `part`; limit is the
// partition's size (compact) or the end of the record's block (blocked), and
// the whole record must end at or below it (the caller knows its length only
// after reading the header).  !ok is BSDB_GET_BAD_ADDR.
struct GetRecord {
    bool ok;
    uint32_t part;
    uint64_t pos, limit;
};

BSDB_HD inline GetRecord get_decode(uint64_t addr, int format, const uint64_t *sizes, uint32_t partitions) {
    GetRecord r = {false, 0, 0, 0};
    if (addr >> 63) return r;                 // SyncReader.java:52: addr < 0 is null
    r.part = (uint32_t)(addr >> 56);          // PartitionedKVReader.java:79
    if (r.part >= partitions) return r;
    const uint64_t size = sizes[r.part];
    if (format == 0) {
        r.pos = addr & 0xFFFFFFFFFFFFFFull;   // PartitionedKVReader.java:80
        r.limit = size;
        r.ok = size >= 3 && r.pos <= size - 3;
        return r;
    }
    const uint64_t block = ((addr >> 16) & 0xFFFFFFFFull) * GET_PAGE;  // BlockedKVReader.java:42-44 (< 2^44)
    const uint64_t bytes = ((addr >> 48) & 0xFFull) * GET_PAGE;        // :46-48 (< 2^20)
    const uint64_t rec = addr & 0xFFFFull;                             // :50-52
    r.pos = block + rec;
    r.limit = block + bytes;
    r.ok = bytes != 0 && r.limit <= size && rec + 3 <= bytes;
    return r;
}

}  // namespace bsdb
