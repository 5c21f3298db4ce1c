// tri_state.cpp -- rt::TriState (raytracercpp_amd/csrc/tri_state.hpp, included alone and compiled as plain
// C++) against the five booleans the renderer kept before the type existed: every transition from every
// reachable state, each compared with what the renderer's code path assigned, and the faults' stickiness.
// Prints "ok <states> <checks>".
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../raytracercpp_amd/csrc/tri_state.hpp"

using rt::TriState;

// the renderer's flags before: d_tri9_ current, tri_ stale, the two faults, the ingest word unread
struct Old {
    bool cur = false, stale = false, nonfin = false, bad = false, live = false;
};

static void drop(Old& o) { o = Old(); }   // drop_device_positions

enum Tr { HOST_REPLACED, INGESTED, EDIT_QUEUED, HOST_EDITED, UPLOADED, DOWNLOADED, INGEST_WORD, EDIT_WORD, NTR };

// the assignments of the code path behind each transition
static void old_step(Old& o, int tr, uint32_t bits)
{
    switch (tr) {
    case HOST_REPLACED: drop(o); break;                                     // set_triangles, clear_geometry, mirror_from
    case INGESTED: o.cur = o.stale = true; o.nonfin = o.bad = false; o.live = true; break;   // ingest_positions
    case EDIT_QUEUED: o.stale = true; break;                                // set_object_transform, device path
    case HOST_EDITED: { const bool b = o.bad; drop(o); o.bad = b; } break;  // set_object_transform, host path
    case UPLOADED: o.cur = true; break;                                     // build_octree_device, launch_raster
    case DOWNLOADED: o.stale = false; break;                                // host_tris
    case INGEST_WORD: o.live = false; o.nonfin = o.nonfin || (bits & 1u); o.bad = o.bad || (bits & 2u); break;
    case EDIT_WORD: o.nonfin = o.nonfin || bits != 0; break;                // apply_device_edits
    }
}

static void new_step(TriState& s, int tr, uint32_t bits)
{
    switch (tr) {
    case HOST_REPLACED: s.host_replaced(); break;
    case INGESTED: s.ingested(); break;
    case EDIT_QUEUED: s.edit_queued(); break;
    case HOST_EDITED: s.host_edited(); break;
    case UPLOADED: s.uploaded(); break;
    case DOWNLOADED: s.downloaded(); break;
    case INGEST_WORD: s.ingest_word(bits); break;
    case EDIT_WORD: s.edit_word(bits); break;
    }
}

static long checks = 0;

static void expect(bool ok, const char* what, int tr)
{
    checks++;
    if (!ok) {
        std::printf("FAIL %s (transition %d)\n", what, tr);
        std::exit(1);
    }
}

static void same(const TriState& s, const Old& o, int tr)
{
    expect(!(o.stale && !o.cur), "the old flags are one of the three legal places", tr);
    expect(s.device_current() == o.cur, "device copy current", tr);
    expect(s.host_current() == !o.stale, "host copy current", tr);
    expect(s.nonfinite() == o.nonfin, "non-finite fault", tr);
    expect(s.bad_index() == o.bad, "bad-index fault", tr);
    expect(s.ingest_unread() == o.live, "ingest word unread", tr);
    const TriState::Where w = o.stale ? TriState::Where::Device : o.cur ? TriState::Where::Both : TriState::Where::Host;
    expect(s.where() == w, "place", tr);
}

static int key(const TriState& s)
{
    return (int)s.where() | s.nonfinite() << 2 | s.bad_index() << 3 | s.ingest_unread() << 4;
}

int main()
{
    struct Node {
        TriState s;
        Old o;
    };
    std::vector<Node> todo{Node{}};
    std::set<int> seen{key(TriState())};
    same(todo[0].s, todo[0].o, -1);
    for (size_t i = 0; i < todo.size(); i++) {
        for (int tr = 0; tr < NTR; tr++) {
            for (uint32_t bits = 0; bits < 4; bits++) {
                if (bits && tr != INGEST_WORD && tr != EDIT_WORD)
                    continue;
                Node n = todo[i];
                if (tr == EDIT_QUEUED && !n.s.device_current()) {
                    // (the renderer queues only while the positions are resident: the illegal fourth
                    // combination is what the old flags would hold here; the type stays where it is)
                    n.s.edit_queued();
                    expect(key(n.s) == key(todo[i].s), "edit_queued without a device copy changes nothing", tr);
                    continue;
                }
                const TriState before = n.s;
                old_step(n.o, tr, bits);
                new_step(n.s, tr, bits);
                same(n.s, n.o, tr);
                // the faults stick: only new positions clear them, and the host-path edit keeps the bad index
                const bool replaces = tr == HOST_REPLACED || tr == INGESTED;
                if (replaces)
                    expect(!n.s.nonfinite() && !n.s.bad_index(), "new positions clear both faults", tr);
                else if (tr == HOST_EDITED)
                    expect(!n.s.nonfinite() && n.s.bad_index() == before.bad_index(), "host edit keeps the bad index alone", tr);
                else
                    expect((n.s.nonfinite() || !before.nonfinite()) && (n.s.bad_index() || !before.bad_index()),
                           "a fault sticks", tr);
                if (tr == INGEST_WORD)
                    expect(n.s.nonfinite() == (before.nonfinite() || (bits & 1u)) &&
                               n.s.bad_index() == (before.bad_index() || (bits & 2u)) && !n.s.ingest_unread(),
                           "the ingest word's bits", tr);
                if (tr == EDIT_WORD)
                    expect(n.s.nonfinite() == (before.nonfinite() || bits != 0) && n.s.bad_index() == before.bad_index(),
                           "the edit word", tr);
                if (seen.insert(key(n.s)).second)
                    todo.push_back(n);
            }
        }
    }
    std::printf("ok %zu %ld\n", todo.size(), checks);
    return 0;
}
