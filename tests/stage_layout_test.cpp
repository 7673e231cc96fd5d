// CPU unit test of the staging layout of host-memory calls (pyfft_amd/csrc/stage.h); built and run by
// tests/test_host_cpu.py::test_stage_layout with g++ (no HIP).  The "scratch buffers" are malloc'ed bytes of exactly the planned
// size, so that a piece reaching past its scratch is an AddressSanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "stage.h"

using namespace sp;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            exit(1);                                                     \
        }                                                                \
    } while (0)

// what spectral.hip's Stage::commit does with a plan: one buffer of `total` bytes per scratch, every piece's pointer into its slot.
// Paints every piece with its index + 1 and fails when a byte is painted twice.
struct Buffers {
    std::vector<unsigned char *> base;
    explicit Buffers(StagePlan &p) {
        for (int a = 0; a < p.nareas; ++a) {
            base.push_back((unsigned char *)calloc(p.area[a].total ? p.area[a].total : 1, 1));
            p.seal(a);
        }
        for (int i = 0; i < p.npieces; ++i) {
            const StagePlan::Piece &q = p.piece[i];
            CHECK(q.off == 0 || q.off % StagePlan::kAlign == 0);
            CHECK(q.off + q.bytes <= p.area[q.area].total);
            unsigned char *d = base[(size_t)q.area] + q.off;
            for (size_t j = 0; j < q.bytes; ++j) {
                CHECK(d[j] == 0);
                d[j] = (unsigned char)(i + 1);
            }
            if (q.slot) memcpy(q.slot, &d, sizeof d);
        }
    }
    ~Buffers() {
        for (unsigned char *b : base) free(b);
    }
};

static const size_t kSizes[] = {0, 1, 255, 256, 257};
static int keyA, keyB, keyC;          // identities of three scratch buffers
static char host[8][4096];            // host arrays to register

// sizes 0, 1, 255, 256, 257 in every order of two, as inputs and outputs of one scratch and of two
static void test_sizes() {
    for (size_t s0 : kSizes)
        for (size_t s1 : kSizes)
            for (size_t s2 : kSizes) {
                StagePlan p;
                void *d0 = nullptr, *d1 = nullptr, *d2 = nullptr, *d3 = nullptr;
                const int i0 = p.add(&keyA, host[0], nullptr, s0, &d0);
                const int i1 = p.add(&keyA, nullptr, host[1], s1, &d1);
                const int i2 = p.add(&keyB, host[2], nullptr, s2, &d2);
                const int i3 = p.add(&keyA, host[3], host[3], s2, &d3);          // in place: copied in and back
                CHECK(!p.err && i0 == 0 && i1 == 1 && i2 == 2 && i3 == 3 && p.nareas == 2 && p.npieces == 4);
                CHECK(p.piece[0].off == 0 && p.piece[2].off == 0);                 // the first piece of a scratch stays at its base
                CHECK(p.piece[1].off >= s0 && p.piece[1].off < s0 + StagePlan::kAlign + (s0 == 0));
                CHECK(p.area[0].total == p.piece[3].off + s2 && p.area[1].total == s2);
                Buffers b(p);
                CHECK(d0 == b.base[0] && d2 == b.base[1] && d1 == b.base[0] + p.piece[1].off && d3 == b.base[0] + p.piece[3].off);
                // copy-back list: the output and the in-place piece, in registration order, with their byte counts
                int k = p.next_back(-1);
                CHECK(k == 1 && p.piece[k].to == host[1] && p.piece[k].bytes == s1);
                k = p.next_back(k);
                CHECK(k == 3 && p.piece[k].to == host[3] && p.piece[k].bytes == s2 && p.piece[k].from == host[3]);
                CHECK(p.next_back(k) == -1);
            }
}

// the four optional outputs of sp_cwt (W, gws, recon, bandpow) and of sp_ssq (T, P, IF, GD) behind one input, every subset present
static void test_four_outputs(const size_t bytes[4]) {
    for (int m = 0; m < 16; ++m) {
        StagePlan p;
        void *x = nullptr, *d[4] = {&x, &x, &x, &x};                    // not null before: an absent piece must not leave them so
        CHECK(p.add(&keyA, host[0], nullptr, 1600, &x) == 0);
        int want[4], nwant = 0;
        for (int k = 0; k < 4; ++k) {
            const bool present = (m >> k) & 1;
            const int idx = p.add(&keyB, nullptr, present ? host[1 + k] : nullptr, bytes[k], &d[k]);
            if (present) want[nwant++] = idx;
            else {
                CHECK(idx == -1);
                d[k] = nullptr;                                          // what the executor hands out for an absent piece
            }
        }
        CHECK(!p.err && p.npieces == 1 + nwant && p.nareas == (nwant ? 2 : 1));
        Buffers b(p);                                                    // (overlap, alignment and the totals are checked in here)
        size_t end = 0;
        int back = -1;
        for (int j = 0, k = 0; k < 4; ++k) {
            if (!((m >> k) & 1)) {
                CHECK(d[k] == nullptr);
                continue;
            }
            const StagePlan::Piece &q = p.piece[want[j]];
            CHECK(d[k] == b.base[1] + q.off && q.bytes == bytes[k] && q.to == host[1 + k] && q.from == nullptr);
            CHECK(j == 0 ? q.off == 0 : q.off >= end);                   // in order, the first at the scratch's base
            end = q.off + q.bytes;
            back = p.next_back(back);
            CHECK(back == want[j]);
            ++j;
        }
        CHECK(p.next_back(back) == -1);
        if (nwant) CHECK(p.area[1].total == end);
    }
}

static void test_refusals() {
    {   // more pieces than the capacity: refused, nothing written past the arrays (ASan would say), the error sticks
        StagePlan p;
        for (int i = 0; i < StagePlan::kMaxPieces; ++i) CHECK(p.add(&keyA, host[0], nullptr, 8) == i);
        CHECK(!p.err);
        CHECK(p.add(&keyA, host[0], nullptr, 8) == -1 && p.err && p.npieces == StagePlan::kMaxPieces);
        const char *first = p.err;
        CHECK(p.add(&keyB, host[0], nullptr, 8) == -1 && p.err == first);
    }
    {   // more scratch buffers than the capacity
        StagePlan p;
        static int keys[StagePlan::kMaxAreas + 1];
        for (int a = 0; a < StagePlan::kMaxAreas; ++a) CHECK(p.add(&keys[a], host[0], nullptr, 8) == a);
        CHECK(p.add(&keys[StagePlan::kMaxAreas], host[0], nullptr, 8) == -1 && p.err && p.nareas == StagePlan::kMaxAreas);
    }
    {   // sums that leave size_t: the aligned offset, and the offset plus the size
        StagePlan p;
        CHECK(p.add(&keyA, host[0], nullptr, SIZE_MAX - 100) == 0 && !p.err);
        CHECK(p.add(&keyA, host[0], nullptr, 1) == -1 && p.err);
        StagePlan q;
        CHECK(q.add(&keyA, host[0], nullptr, 1000) == 0 && q.add(&keyA, host[0], nullptr, SIZE_MAX - 1000) == -1 && q.err);
        CHECK(q.area[0].total == 1000 && q.npieces == 1);               // a refused piece changes nothing
        StagePlan r;
        CHECK(r.add(&keyA, host[0], nullptr, SIZE_MAX) == 0 && !r.err && r.area[0].total == SIZE_MAX);
    }
    {   // a scratch that has been sized takes no further piece (its buffer could move under the pointers handed out); others do
        StagePlan p;
        CHECK(p.add(&keyA, host[0], nullptr, 64) == 0);
        p.seal(0);
        CHECK(p.add(&keyB, nullptr, host[1], 64) == 1 && !p.err);
        CHECK(p.add(&keyA, nullptr, host[2], 64) == -1 && p.err);
    }
    {   // absent pieces: no room, no copy-back, no scratch opened for them
        StagePlan p;
        CHECK(p.add(&keyC, nullptr, nullptr, 1 << 20) == -1 && !p.err && p.npieces == 0 && p.nareas == 0 && p.next_back(-1) == -1);
    }
    {   // zero-byte pieces: registered, in the copy-back list with zero bytes, and harmless to their neighbours
        StagePlan p;
        void *d[3];
        CHECK(p.add(&keyA, nullptr, host[0], 0, &d[0]) == 0 && p.add(&keyA, nullptr, host[1], 0, &d[1]) == 1 &&
              p.add(&keyA, nullptr, host[2], 5, &d[2]) == 2 && !p.err);
        CHECK(p.piece[0].off == 0 && p.piece[1].off == 0 && p.piece[2].off == 0 && p.area[0].total == 5);
        Buffers b(p);
        CHECK(p.next_back(-1) == 0 && p.next_back(0) == 1 && p.next_back(1) == 2 && p.next_back(2) == -1);
    }
}

int main() {
    test_sizes();
    // sp_cwt on 2 rows of 400 float32 samples at 3 scales: W complex64 [2][3][400], gws float64 [2][3], recon complex64 [2][400],
    // bandpow float32 [2][400]; sp_ssq on 2 rows, 15 frames of 33 bins: T complex64, P / IF / GD float32
    const size_t cwt[4] = {8 * 2 * 3 * 400, 8 * 2 * 3, 8 * 2 * 400, 4 * 2 * 400};
    const size_t ssq[4] = {8 * 2 * 15 * 33, 4 * 2 * 15 * 33, 4 * 2 * 15 * 33, 4 * 2 * 15 * 33};
    const size_t odd[4] = {1, 255, 257, 0};
    test_four_outputs(cwt);
    test_four_outputs(ssq);
    test_four_outputs(odd);
    test_refusals();
    printf("stage layout ok\n");
    return 0;
}
