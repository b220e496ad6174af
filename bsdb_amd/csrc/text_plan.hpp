// text_plan.hpp -- what the text front end (capi_text.hip, text_kernels.hip)
// allocates and launches, decided on the host from plain numbers: the grids
// (the packs' is piece_grid, piece_plan.hpp), the most records a chunk can hold (text_max_records), a chunk's device
// footprint once its lines and separators are counted (text_footprint), the
// chunk size (text_chunk_bytes), the runs of the partition rule
// (text_run_bound), where a buffer of a file is cut (text_cut), and the
// verdict on one line (text_verdict), which the records kernel calls too; for
// the blocked layout the placement rule stated sequentially
// (text_place_blocked), the image's bound (text_image_max_blocked) and the
// footprint and chunk size with the placement's workspace.
// C++17 without HIP or getenv, so the arithmetic runs (and is checked,
// tests/text_plan_check.cpp) without a GPU.
//   tools/Builder.java:144-176 (BufferedReader.lines, String.split(sep), put)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "piece_plan.hpp"  // the packs' grid (piece_grid); BSDB_HD

namespace bsdb {

constexpr uint64_t TEXT_MAX_BYTES = 0xFFFFFFFFull;       // a chunk is shorter than 2^32 bytes: positions are u32
constexpr uint64_t TEXT_GRID_MAX = 0xFFFFFFFFull;        // a launch's workgroups stay below 2^32
constexpr uint32_t TEXT_BLOCK_BYTES = 4096;              // k_text_count / positions: 256 threads x one 16-byte piece
constexpr uint32_t TEXT_MAX_KEY = 255;                   // Common.MAX_KEY_SIZE
constexpr uint32_t TEXT_MAX_VALUE = 32510;               // Common.MAX_VALUE_SIZE
constexpr int TEXT_MAX_PARTS = 128;                      // addr >>> 56 of a non-negative address
constexpr uint64_t TEXT_MAX_FILE = 1ull << 56;           // a partition file's offsets are 56 bits
constexpr uint64_t TEXT_DEFAULT_CHUNK = 256ull << 20;
constexpr uint64_t TEXT_MIN_CHUNK = 64ull << 10;

enum TextWord {
    TW_LINES = 0, TW_RECORDS, TW_NOT_TWO_FIELDS, TW_EMPTY_KEY, TW_TOO_LARGE, TW_KEY_BYTES, TW_VALUE_BYTES, TW_MAX_KEY_LEN,
    TW_MAX_VALUE_LEN, TW_CHUNKS, TW_WORDS
};
enum TextVerdict { TV_KEPT = 0, TV_NOT_TWO_FIELDS = 1, TV_EMPTY_KEY = 2, TV_TOO_LARGE = 3 };

// A kept record takes at least 4 bytes of text (key, separator, value,
// terminator), the last one of a text 3: at most bytes / 4 + 1 records.
BSDB_HD inline uint64_t text_max_records(uint64_t bytes) { return bytes / 4 + 1; }

// The image of a chunk: a record is its text (key, separator, value,
// terminator: >= 4 bytes) with the separator and the terminator replaced by
// the 3-byte header, so one byte longer (two for an unterminated last line):
// <= bytes + bytes / 4 + 2, kept below 1.5 x the chunk.  The key blob holds
// bytes of the text only.
inline uint64_t text_image_max(uint64_t bytes) { return bytes + bytes / 2 + 16; }
inline uint64_t text_blob_max(uint64_t bytes) { return bytes + 16; }

// k_text_count / k_text_positions: a workgroup per TEXT_BLOCK_BYTES of text
inline uint64_t text_blocks(uint64_t bytes) { return (bytes >> 12) + ((bytes & 4095) != 0); }
inline uint32_t text_count_grid(uint64_t bytes) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(text_blocks(bytes), TEXT_GRID_MAX));
}

// a line, or a record, per lane, grid-stride
inline uint32_t text_lane_grid(uint64_t items, int num_cus) {
    const uint64_t cus = (uint64_t)std::max(1, num_cus);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(items >> 8) + ((items & 255) != 0), cus * 16, TEXT_GRID_MAX}));
}

// Device bytes of one chunk of `bytes` text bytes with `lines` lines and
// `seps` separator bytes (both <= bytes): the split's workspace (per-block
// counts and their scans, the two position lists, the keep flags and their
// scan), the descriptors and the pack's outputs and scans at the most records
// the chunk can hold.  bytes < 2^32, so the sum stays below 2^40.
struct TextFootprint {
    uint64_t split = 0;  // workspace of the split
    uint64_t pack = 0;   // descriptors, size scans, image, key blob + offsets, addresses, value heads
    uint64_t total = 0;  // both, and the text itself (+16 B of slack)
};

inline TextFootprint text_footprint(uint64_t bytes, uint64_t lines, uint64_t seps, bool approximate) {
    TextFootprint f;
    const uint64_t nb = std::max<uint64_t>(1, text_blocks(bytes)), r = text_max_records(bytes);
    f.split = 2 * 4 * nb + 2 * 8 * (nb + 1) + 4 * lines + 4 * (seps + 1) + 4 * lines + 8 * (lines + 1);
    f.pack = 4 * 4 * r + 2 * 4 * r + 2 * 8 * (r + 1) + text_image_max(bytes) + text_blob_max(bytes) + 8 * (r + 1) + 8 * r +
             (approximate ? 9 * r : 0);
    f.total = bytes + 16 + f.split + f.pack;
    return f;
}

// The chunk size: what the caller asked for (0 = default), at least
// TEXT_MIN_CHUNK, below 2^32, and halved until the footprint of a chunk whose
// every byte is a line and a separator (more than any text has) fits half of
// the free memory.
inline uint64_t text_chunk_bytes(uint64_t requested, uint64_t free_bytes) {
    uint64_t c = requested ? requested : TEXT_DEFAULT_CHUNK;
    c = std::min<uint64_t>(std::max<uint64_t>(c, TEXT_MIN_CHUNK), TEXT_MAX_BYTES & ~15ull);
    while (c > TEXT_MIN_CHUNK && text_footprint(c, c, c, true).total > free_bytes / 2) c = std::max<uint64_t>(TEXT_MIN_CHUNK, c / 2);
    return c;
}

// The partition rule: the k kept records of a chunk are cut into `partitions`
// contiguous runs, run p = records [p k / P, (p + 1) k / P).  k <= 2^30 and
// p <= 128: the product stays below 2^38.
BSDB_HD inline uint64_t text_run_bound(uint64_t k, uint32_t partitions, uint32_t p) { return (uint64_t)p * k / partitions; }

// Where a buffer holding `fill` bytes of a file is cut: the length of the
// largest prefix that ends a line -- after a '\n', or after a '\r' whose next
// byte is in the buffer and is not '\n' (a '\r' as the last byte may be half
// of a "\r\n").  At the end of the file the prefix is everything.  0: the
// buffer holds no line end.
inline uint64_t text_cut(const uint8_t *buf, uint64_t fill, bool eof) {
    if (eof) return fill;
    for (uint64_t i = fill; i > 0; --i) {
        const uint8_t b = buf[i - 1];
        if (b == '\n') return i;
        if (b == '\r' && i < fill && buf[i] != '\n') return i;
    }
    return 0;
}

// ---- the blocked layout (BlockedKVWriter.java:45-74, :134-136) ------------
// One run (the records of one partition in one chunk, in input order) into
// blocks of B bytes appended to a file that holds F bytes.  size = 3 + kLen +
// vLen.  A record with size > B is LARGE: a block of its own of ceil(size /
// 4096) pages, appended at once, ahead of the block that is open.  A small
// record that does not fit the rest of the open block closes it (the block is
// appended at the file's end) and opens a new one; a record that exactly fills
// the block leaves it open.  The run's end closes the open block (deviation 6
// of the header: the reference's block lives on until finish).
constexpr uint32_t TEXT_PAGE = 4096;
constexpr uint32_t TEXT_MAX_BLOCK = 65536;               // the address has 16 bits of offset
constexpr uint64_t TEXT_MAX_FILE_BLOCKED = 1ull << 44;   // ... and 32 bits of pages
constexpr uint32_t TEXT_TILE = 2048;                     // records of one workgroup of the placement kernels
constexpr uint32_t TEXT_MAX_RECORD = 3 + TEXT_MAX_KEY + TEXT_MAX_VALUE;  // 32 768

BSDB_HD inline bool text_bad_block_size(uint32_t B) { return B < TEXT_PAGE || B > TEXT_MAX_BLOCK || (B & (TEXT_PAGE - 1)); }
BSDB_HD inline uint32_t text_large_block(uint32_t size) { return (size + TEXT_PAGE - 1) & ~(TEXT_PAGE - 1); }

struct TextPlaced {
    uint64_t block_pos;    // file position of the record's block
    uint32_t block_bytes;  // B, or a large record's pages
    uint32_t offset;       // of the record in its block
};

// The rule, one record per step: the specification of the placement kernels
// (tests/text_blocked_check.cpp holds it against a byte-level emulation of
// writeRecord / flushBlocks).  Returns the bytes the run appends; `out` may be
// null.  sizes[i] in 4 .. 32 768.
inline uint64_t text_place_blocked(const uint32_t *sizes, uint64_t count, uint32_t B, uint64_t F, TextPlaced *out) {
    uint64_t end = F;          // the file's end
    uint32_t fill = 0;         // bytes in the open block
    bool open = false;
    uint64_t first = 0;        // the open block's first record
    auto close = [&](uint64_t upto) {
        for (uint64_t j = first; out && j < upto; ++j)
            if (sizes[j] <= B) out[j].block_pos = end;
        end += B;
        open = false;
    };
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t size = sizes[i];
        if (size > B) {
            if (out) out[i] = {end, text_large_block(size), 0};
            end += text_large_block(size);
            continue;
        }
        if (open && B - fill < size) close(i);
        if (!open) {
            open = true;
            fill = 0;
            first = i;
        }
        if (out) out[i] = {0, B, fill};
        fill += size;
    }
    if (open) close(count);
    return end - F;
}

// An upper bound of the blocked image of a chunk of `bytes` text bytes.  The
// records themselves take R <= bytes + bytes / 4 + 2 bytes (text_image_max's
// argument).  In one run, the first record of a block did not fit the block
// before it, so two consecutive blocks hold more than B bytes together: n
// blocks of a run that hold Rs bytes have floor(n / 2) disjoint such pairs,
// Rs > (n - 1) / 2 x B, n x B < 2 Rs + B: the last, partial block of each run
// costs at most B, the others at most twice what they hold.  A large record
// (size > B >= 4096) gets less than size + 4096 < 2 x size.  Together:
// < 2 R + partitions x B.
inline uint64_t text_image_max_blocked(uint64_t bytes, int partitions, uint32_t B) {
    return 2 * (bytes + bytes / 4 + 2) + (uint64_t)std::max(1, partitions) * B + 16;
}

// The placement's workspace for r records: the small sizes and their scan,
// next, (last, exit), the events and their scan, each record's block offset
// and block end, the two position lists, and entry + carry per tile.
inline uint64_t text_place_workspace(uint64_t r) {
    const uint64_t tiles = r / TEXT_TILE + 1;
    return 4 * r + 8 * (r + 1) + 4 * r + 8 * r + 4 * r + 8 * (r + 1) + 4 * r + 4 * r + 2 * 8 * (r + 1) + 2 * 4 * tiles + 64;
}

// text_footprint with the blocked image and the placement's workspace: never
// below the compact footprint.
inline TextFootprint text_footprint_blocked(uint64_t bytes, uint64_t lines, uint64_t seps, bool approximate, int partitions,
                                            uint32_t B) {
    TextFootprint f = text_footprint(bytes, lines, seps, approximate);
    const uint64_t more = text_image_max_blocked(bytes, partitions, B) - text_image_max(bytes) +
                          text_place_workspace(text_max_records(bytes));
    f.pack += more;
    f.total += more;
    return f;
}

inline uint64_t text_chunk_bytes_blocked(uint64_t requested, uint64_t free_bytes, int partitions, uint32_t B) {
    uint64_t c = requested ? requested : TEXT_DEFAULT_CHUNK;
    c = std::min<uint64_t>(std::max<uint64_t>(c, TEXT_MIN_CHUNK), TEXT_MAX_BYTES & ~15ull);
    while (c > TEXT_MIN_CHUNK && text_footprint_blocked(c, c, c, true, partitions, B).total > free_bytes / 2)
        c = std::max<uint64_t>(TEXT_MIN_CHUNK, c / 2);
    return c;
}

// The separator: one literal byte below 0x80 that ends no line.
inline bool text_bad_separator(int sep) { return sep < 0 || sep >= 0x80 || sep == '\r' || sep == '\n'; }

// The verdict on the line [start, end) (terminator excluded) that holds `c`
// separator bytes, the first two at s1 < s2 (read only when c >= 1, c >= 2).
// String.split(sep) cuts at every separator and drops trailing empty fields;
// the line is a record iff exactly two fields remain (Builder.java:150-152):
// the value [s1 + 1, c >= 2 ? s2 : end) is not empty, and when c >= 2 all
// bytes from s2 to the end are the other c - 1 separators (end - s2 == c - 1).
// Then: an empty key is dropped (the reference would put it; this project's
// writers take keys of 1..255 bytes), a key over 255 or a value over 32 510
// bytes is too large.
struct TextLine {
    uint32_t verdict;  // TextVerdict
    uint32_t kpos, klen, vpos, vlen;
};

BSDB_HD inline TextLine text_verdict(uint32_t start, uint32_t end, uint32_t c, uint32_t s1, uint32_t s2) {
    TextLine t = {TV_NOT_TWO_FIELDS, 0, 0, 0, 0};
    if (c == 0) return t;
    const uint32_t vend = c >= 2 ? s2 : end;
    if (vend <= s1 + 1) return t;                   // the second field is empty
    if (c >= 2 && end - s2 != c - 1) return t;      // a third field
    t.kpos = start;
    t.klen = s1 - start;
    t.vpos = s1 + 1;
    t.vlen = vend - (s1 + 1);
    t.verdict = t.klen == 0 ? TV_EMPTY_KEY : (t.klen > TEXT_MAX_KEY || t.vlen > TEXT_MAX_VALUE) ? TV_TOO_LARGE : TV_KEPT;
    return t;
}

}  // namespace bsdb
