// text_blocked_check.cpp -- holds text_place_blocked (text_plan.hpp), the
// specification of the blocked placement kernels, against a byte-level
// emulation of BlockedKVWriter's writeRecord / flushBlocks: one B-byte buffer
// with a position, "remaining() < recLen" closes it, a record longer than the
// buffer goes into a page-aligned buffer of its own that is flushed at once.
// The emulation writes a file image; every record is then found in that image
// at the place text_place_blocked gives, and the image's length is the run's
// byte count.  Cases: every sequence of up to 5 sizes from the issue's table
// at B = 4096, and seeded random runs over several B and F.  Also: the image
// never exceeds text_image_max_blocked, and the blocked footprint and chunk
// size never exceed the compact ones' room.  Prints one JSON line; exit code 1
// on the first disagreement.  Built with -fsanitize=address,undefined and run
// by tests/test_text_blocked_plan_cpu.py; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../bsdb_amd/csrc/text_plan.hpp"

using namespace bsdb;

// record i of `size` bytes: every byte i % 255 + 1 (never 0), so a record found at a wrong place shows
static void fill_record(std::vector<uint8_t> &rec, uint64_t i, uint32_t size) { rec.assign(size, (uint8_t)(i % 255 + 1)); }

struct Emulated {
    std::vector<uint8_t> file;
    std::vector<uint64_t> pos;      // block position in the file (F not included)
    std::vector<uint32_t> bbytes, off;
};

static void emulate(const std::vector<uint32_t> &sizes, uint32_t B, Emulated &e) {
    static std::vector<uint8_t> buf, rec, large;  // (kept between calls: the cases are many and small)
    static std::vector<uint64_t> pending, one;     // records in the open buffer; the large record
    buf.assign(B, 0);
    pending.clear();
    uint32_t position = 0;           // tempBuf.position()
    const uint64_t n = sizes.size();
    e.file.clear();
    e.pos.assign(n, 0);
    e.bbytes.assign(n, 0);
    e.off.assign(n, 0);
    auto flush = [&](std::vector<uint8_t> &b, uint32_t &bpos, std::vector<uint64_t> &recs) {  // flushBlocks
        if (bpos == 0) return;
        if (b.size() - bpos > 0) b[bpos] = 0;  // mark data finished
        for (uint64_t r : recs) e.pos[r] = e.file.size();
        e.file.insert(e.file.end(), b.begin(), b.end());
        recs.clear();
    };
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t len = sizes[i];
        fill_record(rec, i, len);
        if (len > B) {  // large records
            large.assign(text_large_block(len), 0);
            memcpy(large.data(), rec.data(), len);
            uint32_t lpos = len;
            one.assign(1, i);
            e.bbytes[i] = (uint32_t)large.size();
            e.off[i] = 0;
            flush(large, lpos, one);
        } else {
            if (B - position < len) {  // tempBuf.remaining() < recLen
                flush(buf, position, pending);
                position = 0;          // tempBuf.clear(); the buffer is reused: zero it as allocateDirect did
                std::fill(buf.begin(), buf.end(), 0);
            }
            memcpy(buf.data() + position, rec.data(), len);
            e.bbytes[i] = B;
            e.off[i] = position;
            pending.push_back(i);
            position += len;
        }
    }
    flush(buf, position, pending);  // the run's end closes the open block
}

static unsigned long long g_runs = 0, g_records = 0, g_max_ratio_pm = 0;

static bool check(const std::vector<uint32_t> &sizes, uint32_t B, uint64_t F) {
    static Emulated e;
    static std::vector<TextPlaced> pl;
    static std::vector<uint8_t> expect;
    emulate(sizes, B, e);
    pl.assign(sizes.size(), TextPlaced{});
    const uint64_t bytes = text_place_blocked(sizes.data(), sizes.size(), B, F, pl.data());
    if (bytes != e.file.size() || bytes % TEXT_PAGE) {
        fprintf(stderr, "run bytes %llu, emulation %zu\n", (unsigned long long)bytes, e.file.size());
        return false;
    }
    if (text_place_blocked(sizes.data(), sizes.size(), B, F, nullptr) != bytes) return false;
    expect.assign(e.file.size(), 0);  // the records at text_place_blocked's places, every other byte 0
    for (uint64_t i = 0; i < sizes.size(); ++i) {
        if (pl[i].block_pos != F + e.pos[i] || pl[i].block_bytes != e.bbytes[i] || pl[i].offset != e.off[i]) {
            fprintf(stderr, "record %llu: (%llu, %u, %u), emulation (%llu, %u, %u)\n", (unsigned long long)i,
                    (unsigned long long)pl[i].block_pos, pl[i].block_bytes, pl[i].offset, (unsigned long long)(F + e.pos[i]),
                    e.bbytes[i], e.off[i]);
            return false;
        }
        const uint64_t at = pl[i].block_pos - F + pl[i].offset;
        if (at + sizes[i] > e.file.size()) return false;
        if (pl[i].offset + (uint64_t)sizes[i] > pl[i].block_bytes || pl[i].block_pos % TEXT_PAGE) return false;
        memset(expect.data() + at, (int)(i % 255 + 1), sizes[i]);
    }
    if (!expect.empty() && memcmp(expect.data(), e.file.data(), expect.size()) != 0) return false;
    ++g_runs;
    g_records += sizes.size();
    return true;
}

int main(int argc, char **) {
    if (argc > 1) return 0;  // (any argument: only show that the program starts)
    // 1. exhaustive: B = 4096, every sequence of up to 5 of these sizes
    const uint32_t table[] = {5, 6, 2047, 2048, 2049, 4091, 4095, 4096, 4097, 8192, 8193, 32768};
    const int T = (int)(sizeof(table) / sizeof(table[0]));
    unsigned long long exhaustive = 0;
    for (int len = 0; len <= 5; ++len) {
        std::vector<int> idx((size_t)len, 0);
        for (;;) {
            std::vector<uint32_t> sizes;
            for (int d : idx) sizes.push_back(table[d]);
            if (!check(sizes, 4096, 0)) return 1;
            ++exhaustive;
            int d = len - 1;
            while (d >= 0 && ++idx[(size_t)d] == T) idx[(size_t)d--] = 0;
            if (d < 0) break;
        }
    }
    // 2. seeded random runs: skewed sizes, several B and F
    std::mt19937_64 rng(20240611);
    const uint32_t Bs[] = {4096, 8192, 16384, 65536};
    unsigned long long random_runs = 0;
    for (int it = 0; it < 400; ++it) {
        const uint32_t B = Bs[it % 4];
        const uint64_t F = (it % 3) ? (uint64_t)(rng() % 1000) * TEXT_PAGE : 0;
        const uint64_t n = rng() % 600;
        std::vector<uint32_t> sizes(n);
        for (uint32_t &s : sizes) {
            const uint64_t r = rng() % 100;
            s = r < 60 ? 5 + (uint32_t)(rng() % 60) : r < 85 ? 5 + (uint32_t)(rng() % 3000)
                : r < 95 ? (B > 64 ? B - 32 + (uint32_t)(rng() % 64) : 5) : 5 + (uint32_t)(rng() % (TEXT_MAX_RECORD - 4));
            s = s > TEXT_MAX_RECORD ? TEXT_MAX_RECORD : s;
        }
        if (!check(sizes, B, F)) return 1;
        ++random_runs;
    }
    // 3. the image bound: the densest texts.  A record of size s >= 5 comes from s - 1 bytes of text (key,
    // separator, value, terminator against the 3-byte header); `parts` runs of records of one size each.
    unsigned long long bound_cases = 0;
    for (uint32_t B : Bs)
        for (int parts : {1, 3, 8, 128})
            for (uint32_t s : {5u, 6u, B / 2 + 1, B / 2, B, B + 1, 4097u, 8193u, 20000u, TEXT_MAX_RECORD}) {
                if (s > TEXT_MAX_RECORD) continue;
                for (uint64_t per_run : {1ull, 2ull, 3ull, 7ull, 100ull}) {
                    std::vector<uint32_t> sizes(per_run, s);
                    const uint64_t run = text_place_blocked(sizes.data(), per_run, B, 0, nullptr);
                    const uint64_t text_bytes = (uint64_t)parts * per_run * (s - 1);
                    const uint64_t image = (uint64_t)parts * run, bound = text_image_max_blocked(text_bytes, parts, B);
                    if (image > bound) {
                        fprintf(stderr, "image %llu over bound %llu (B %u parts %d size %u x %llu)\n", (unsigned long long)image,
                                (unsigned long long)bound, B, parts, s, (unsigned long long)per_run);
                        return 1;
                    }
                    const unsigned long long pm = image * 1000 / bound;
                    g_max_ratio_pm = pm > g_max_ratio_pm ? pm : g_max_ratio_pm;
                    ++bound_cases;
                }
            }
    // the random runs again, as one partition's chunk
    for (int it = 0; it < 200; ++it) {
        const uint32_t B = Bs[it % 4];
        const uint64_t n = 1 + rng() % 2000;
        std::vector<uint32_t> sizes(n);
        uint64_t text_bytes = 0;
        for (uint32_t &s : sizes) {
            s = (rng() % 10) ? 5 + (uint32_t)(rng() % 5000) : 5 + (uint32_t)(rng() % (TEXT_MAX_RECORD - 4));
            text_bytes += s - 1;
        }
        if (text_place_blocked(sizes.data(), n, B, 0, nullptr) > text_image_max_blocked(text_bytes, 1, B)) return 1;
        ++bound_cases;
    }
    // 4. footprint and chunk: blocked >= compact, so a blocked chunk is never larger
    unsigned long long fp_cases = 0;
    for (uint64_t b : {0ull, 1ull, 4096ull, 65536ull, 1ull << 20, 256ull << 20, 0xFFFFFFF0ull})
        for (uint32_t B : Bs)
            for (int parts : {1, 8, 128})
                for (int approx : {0, 1}) {
                    const TextFootprint c = text_footprint(b, b, b, approx), k = text_footprint_blocked(b, b, b, approx, parts, B);
                    if (k.total < c.total || k.pack < c.pack || k.split != c.split || k.total >= (1ull << 41)) return 1;
                    if (text_image_max_blocked(b, parts, B) < text_image_max(b)) return 1;
                    for (uint64_t free_b : {0ull, 1ull << 30, 64ull << 30, 280000000000ull}) {
                        const uint64_t cb = text_chunk_bytes_blocked(b, free_b, parts, B), cc = text_chunk_bytes(b, free_b);
                        if (cb > cc || cb < TEXT_MIN_CHUNK) return 1;
                        if (cb > TEXT_MIN_CHUNK && text_footprint_blocked(cb, cb, cb, true, parts, B).total > free_b / 2) return 1;
                    }
                    ++fp_cases;
                }
    // 5. the limits
    for (uint32_t B : {0u, 1u, 4095u, 6000u, 69632u, 131072u})
        if (!text_bad_block_size(B)) return 1;
    for (uint32_t B = 4096; B <= 65536; B += 4096)
        if (text_bad_block_size(B)) return 1;
    printf("{\"exhaustive\":%llu,\"random_runs\":%llu,\"runs\":%llu,\"records\":%llu,\"bound_cases\":%llu,"
           "\"max_image_permille_of_bound\":%llu,\"footprint_cases\":%llu,\"default_chunk\":%llu}\n",
           exhaustive, random_runs, g_runs, g_records, bound_cases, g_max_ratio_pm, fp_cases,
           (unsigned long long)text_chunk_bytes_blocked(0, 280000000000ull, 8, 4096));
    return 0;
}
