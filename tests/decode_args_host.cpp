// Host program of tests/test_file_reader_cpu.py: egogaussian_amd/csrc/decode_args.h, the argument checks the PNG and JPEG entries share,
// compiled by the host compiler with -fsanitize=address,undefined.  Every case states the decision the entries' own three-condition lines
// gave before the header existed: the stated `want` of each case is what the test rests on.  `lines` below restates those lines in their
// own order (sizes first), a second opinion over many pairings.  The program prints each disagreement and exits 1 when there is one.
#include <cstdint>
#include <cstdio>

#include "../egogaussian_amd/csrc/decode_args.h"

static int failures = 0;

// the lines of the entries: sizes first, then alignment, order and offset > limit - room
static bool lines(uint64_t offset, uint64_t room, uint64_t align, uint64_t limit, size_t* end) {
    if (room > limit) return false;
    if ((offset & (align - 1)) || offset < *end || offset > limit - room) return false;
    *end = (size_t)(offset + room);
    return true;
}

static void region(const char* what, uint64_t offset, uint64_t room, uint64_t align, uint64_t limit, size_t end_before, bool want) {
    size_t end = end_before, end_lines = end_before;
    const bool got = decode_region(offset, room, align, limit, &end), old = lines(offset, room, align, limit, &end_lines);
    const size_t end_want = want ? (size_t)(offset + room) : end_before;
    if (got != want || old != want || end != end_want || end_lines != end_want) {
        printf("region, %s: accepted %d (the lines %d), expected %d; end %zu (the lines %zu), expected %zu\n", what, (int)got, (int)old, (int)want,
               end, end_lines, end_want);
        failures++;
    }
}

static void open(const char* what, int got, int want) {
    if (got != want) {
        printf("opening check, %s: %d, expected %d\n", what, got, want);
        failures++;
    }
}

int main() {
    const uint64_t top = ~(uint64_t)0;                                // 2^64 - 1
    // two regions of 1024 bytes in a buffer of 4096
    region("the first region", 0, 1024, 16, 4096, 0, true);
    region("the second region behind the first", 1024, 1024, 16, 4096, 1024, true);
    region("the second region at offset 0, over the first", 0, 1024, 16, 4096, 1024, false);
    region("the second region inside the first", 16, 1024, 16, 4096, 1024, false);
    region("the second region inside the first, unaligned regions", 100, 1024, 1, 4096, 1024, false);
    region("a misaligned offset", 1032, 1024, 16, 4096, 1024, false);
    region("the same offset where no alignment is asked", 1032, 1024, 1, 4096, 1024, true);
    region("room > limit", 0, 8192, 16, 4096, 0, false);
    region("room == limit", 0, 4096, 16, 4096, 0, true);
    region("offset limit - room", 4096 - 1024, 1024, 16, 4096, 1024, true);
    region("offset limit - room + 16", 4096 - 1024 + 16, 1024, 16, 4096, 1024, false);
    region("an offset past the buffer", (uint64_t)1 << 20, 1024, 16, 4096, 1024, false);
    region("an empty region at the end", 4096, 0, 16, 4096, 1024, true);
    // the wrapping offsets of the GPU tests' tables: offset + room passes 2^64
    region("offset 2^64 - 16", top - 15, 1024, 1, 65536, 1024, false);
    region("offset 2^64 - 1024", top - 1023, 1024, 16, 32768, 0, false);
    region("offset 2^64 - 4096", top - 4095, 4096, 16, 32768, 1024, false);
    region("offset 2^64 - 2^30", top - (((uint64_t)1 << 30) - 1), 1024, 16, 32768, 1024, false);
    region("offset 2^64 - 16, a room that wraps to the start", top - 15, 16, 16, 4096, 0, false);
    // every pairing of these values decides as the lines do
    const uint64_t values[] = {0, 1, 15, 16, 17, 100, 1024, 1032, 3072, 3088, 4096, 8192, (uint64_t)1 << 20, ((uint64_t)1 << 32) - 16, (uint64_t)1 << 32,
                               top - (((uint64_t)1 << 30) - 1), top - 4095, top - 1023, top - 15, top};
    const uint64_t aligns[] = {1, 16};
    const uint64_t ends[] = {0, 16, 1024, 4096};
    int pairings = 0;
    for (uint64_t offset : values)
        for (uint64_t room : values)
            for (uint64_t limit : values)
                for (uint64_t align : aligns)
                    for (uint64_t before : ends) {
                        size_t a = (size_t)before, b = (size_t)before;
                        const bool got = decode_region(offset, room, align, limit, &a), old = lines(offset, room, align, limit, &b);
                        if (got != old || a != b || (!got && a != before)) {
                            printf("region: offset %llu room %llu align %llu limit %llu end %llu: %d against the lines' %d\n", (unsigned long long)offset,
                                   (unsigned long long)room, (unsigned long long)align, (unsigned long long)limit, (unsigned long long)before, (int)got, (int)old);
                            failures++;
                        }
                        pairings++;
                    }

    // the opening check: eight pointers into an aligned buffer
    alignas(64) static unsigned char mem[8][64];
    const void* p[8];
    const char* names[8] = {"files", "desc_host", "desc_device", "second_host", "second_device", "out", "status", "scratch"};
    auto call = [&](int n_files, int n_second, uintptr_t second_align) {
        return decode_open(n_files, n_second, p[0], p[1], p[2], p[3], p[4], second_align, p[5], p[6], p[7]);
    };
    auto reset = [&]() {
        for (int k = 0; k < 8; k++) p[k] = mem[k];
    };
    reset();
    open("accepted", call(1, 1, 4), 0);
    open("n_files 65535", call(65535, 1, 8), 0);
    open("n_files 0", call(0, 1, 4), EGS_ERR_ARG);
    open("n_files -1", call(-1, 1, 4), EGS_ERR_ARG);
    open("n_files 65536", call(65536, 1, 4), EGS_ERR_RANGE);
    open("the second count 0", call(1, 0, 4), EGS_ERR_ARG);
    open("n_files 65536 and the second count 0", call(65536, 0, 4), EGS_ERR_ARG);      // (the counts come before the range)
    for (int k = 0; k < 8; k++) {
        reset();
        p[k] = nullptr;
        char what[64];
        snprintf(what, sizeof what, "NULL %s", names[k]);
        open(what, call(1, 1, 4), EGS_ERR_ARG);
        snprintf(what, sizeof what, "NULL %s with n_files 65536", names[k]);
        open(what, call(65536, 1, 4), EGS_ERR_RANGE);                 // (the range comes before the pointers)
    }
    const struct { int k; int shift; uintptr_t second_align; int want; const char* what; } moved[] = {
        {7, 4, 4, EGS_ERR_ARG, "scratch + 4"}, {7, 8, 4, EGS_ERR_ARG, "scratch + 8"}, {7, 16, 4, 0, "scratch + 16"},
        {6, 2, 4, EGS_ERR_ARG, "status + 2"}, {6, 4, 4, 0, "status + 4"},
        {2, 4, 4, EGS_ERR_ARG, "desc_device + 4"}, {2, 8, 4, 0, "desc_device + 8"},
        {4, 2, 4, EGS_ERR_ARG, "second_device + 2, aligned to 4"}, {4, 4, 4, 0, "second_device + 4, aligned to 4"},
        {4, 4, 8, EGS_ERR_ARG, "second_device + 4, aligned to 8"}, {4, 8, 8, 0, "second_device + 8, aligned to 8"},
        {0, 1, 4, 0, "files + 1"}, {1, 1, 4, 0, "desc_host + 1"}, {3, 1, 4, 0, "second_host + 1"}, {5, 1, 4, 0, "out + 1"}};
    for (const auto& m : moved) {
        reset();
        p[m.k] = mem[m.k] + m.shift;
        open(m.what, call(1, 1, m.second_align), m.want);
    }
    if (up16(0) != 0 || up16(1) != 16 || up16(16) != 16 || up16(17) != 32 || up16(((size_t)1 << 32) - 1) != (size_t)1 << 32) {
        printf("up16\n");
        failures++;
    }
    printf("%d pairings, %d failures\n", pairings, failures);
    return failures ? 1 : 0;
}
