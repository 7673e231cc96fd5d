// stage.h -- the layout of one host-memory (mem = 0) call's staged pieces inside the library's device scratch buffers.
// Pure host logic with no HIP calls, so that the layout rules are unit-tested on the CPU (tests/stage_layout_test.cpp);
// spectral.hip's Stage supplies the buffers, the copies and the synchronisation.
//
// Rules: the pieces of one scratch are laid out in registration order; the first starts at offset 0 (kernels choose
// vector forms from a pointer's low bits, and a scratch's base is what they were handed before), every later one at the
// next multiple of 256 bytes.  An absent piece (null host pointer) takes no room, is never copied and yields a null
// device pointer.  A piece with a host source is copied in, one with a host destination is copied back, one with both
// is transformed in place.  Nothing is allocated: capacities are fixed, and running over one -- or over size_t in the
// sums -- is reported through `err`, never undefined behaviour.  A scratch whose buffer has been sized (seal) takes no
// further piece, so no pointer handed out earlier can be reallocated away.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sp {

struct StagePlan {
    static constexpr int kMaxPieces = 16, kMaxAreas = 6;
    static constexpr size_t kAlign = 256;

    struct Piece {
        const void *from;   // host source, copied in (null: output only)
        void *to;           // host destination, copied back (null: input only)
        size_t bytes, off;  // size and byte offset inside its area
        int area;
        void *slot, *slot2; // the executor's cookies: where the piece's device pointer goes (slot2: a second place, or null)
    };
    struct Area {
        const void *key;    // identity of the scratch buffer
        size_t total;       // bytes the scratch needs
        int npieces;
        bool sealed;
    };
    Piece piece[kMaxPieces];
    Area area[kMaxAreas];
    int npieces = 0, nareas = 0;
    const char *err = nullptr;   // first refusal (sticky)

    // registers a piece; returns its index, or -1 if it is absent or refused (then `err` says why)
    int add(const void *key, const void *from, void *to, size_t bytes, void *slot = nullptr, void *slot2 = nullptr) {
        if (!from && !to) return -1;
        int a = 0;
        while (a < nareas && area[a].key != key) ++a;
        if (a == nareas) {
            if (nareas == kMaxAreas) return refuse("more scratch buffers than a call may stage in");
            area[nareas++] = Area{key, 0, 0, false};
        }
        Area &A = area[a];
        if (A.sealed) return refuse("a piece was added to a scratch buffer that is already sized");
        if (npieces == kMaxPieces) return refuse("more pieces than a call may stage");
        size_t off = 0;
        if (A.npieces) {
            if (A.total > SIZE_MAX - (kAlign - 1)) return refuse("staged sizes overflow size_t");
            off = (A.total + (kAlign - 1)) & ~(kAlign - 1);
        }
        if (bytes > SIZE_MAX - off) return refuse("staged sizes overflow size_t");
        A.total = off + bytes;
        ++A.npieces;
        piece[npieces] = Piece{from, to, bytes, off, a, slot, slot2};
        return npieces++;
    }
    void seal(int a) { area[a].sealed = true; }

    // the copy-back list: pieces with a host destination, in registration order.  next_back(-1) is the first, -1 the end
    int next_back(int i) const {
        for (++i; i < npieces; ++i)
            if (piece[i].to) return i;
        return -1;
    }

private:
    int refuse(const char *why) {
        if (!err) err = why;
        return -1;
    }
};

}   // namespace sp
