// tri_state.hpp -- where the triangle positions currently are, and what is known to be wrong with them.
// No HIP in here: the transitions are checked on their own (tests/c/tri_state.cpp).  TriGeometry
// (tri_geometry.hpp) holds the one instance and is the only caller of the transitions.
//
//   Host   --uploaded-->    Both  --edit_queued-->  Device  --downloaded-->  Both
//   any    --ingested-->    Device                  any --host_replaced / host_edited--> Host
//
// Host: only the host copy is current.  Both: the device copy holds the same positions.  Device: the device
// copy (with the queued edits) is the truth and the host copy is stale.  "Stale host copy, no device copy"
// cannot be written down.
#pragma once

#include <stdint.h>

namespace rt {

class TriState {
public:
    enum class Where : uint8_t { Host, Both, Device };
    Where where() const { return where_; }
    bool host_current() const { return where_ != Where::Device; }
    bool device_current() const { return where_ != Where::Host; }
    // the two faults, sticky until the geometry is replaced: a non-finite coordinate written by a kernel (a host
    // copy that is the truth is scanned instead), and a device input's index out of range
    bool nonfinite() const { return nonfinite_; }
    bool bad_index() const { return bad_index_; }
    bool ingest_unread() const { return ingest_unread_; }   // the last device input's word has not been read

    // new positions given on the host (set_triangles, clear_geometry, a helper's mirror)
    void host_replaced() { *this = TriState(); }
    // new positions written by the device input's kernel: its word is read later (ingest_word)
    void ingested()
    {
        where_ = Where::Device;
        nonfinite_ = bad_index_ = false;
        ingest_unread_ = true;
    }
    // a matrix was queued for the device copy (only while that copy is current)
    void edit_queued() { where_ = where_ == Where::Both ? Where::Device : where_; }
    // the up-to-date host copy was transformed in place: a bad index stays (it left zeros behind, which no
    // host scan can tell from the caller's), the rest describes positions that are gone
    void host_edited()
    {
        const bool bad = bad_index_;
        *this = TriState();
        bad_index_ = bad;
    }
    void uploaded() { where_ = where_ == Where::Host ? Where::Both : where_; }       // the device copy was written
    void downloaded() { where_ = where_ == Where::Device ? Where::Both : where_; }   // the host copy was written
    // the device input's word: bit 0 a non-finite coordinate, bit 1 an index out of range
    void ingest_word(uint32_t bits)
    {
        ingest_unread_ = false;
        nonfinite_ = nonfinite_ || (bits & 1u) != 0;
        bad_index_ = bad_index_ || (bits & 2u) != 0;
    }
    // the transform kernel's word: not 0 when it wrote a non-finite coordinate
    void edit_word(uint32_t bits) { nonfinite_ = nonfinite_ || bits != 0; }

private:
    Where where_ = Where::Host;
    bool nonfinite_ = false, bad_index_ = false, ingest_unread_ = false;
};

}  // namespace rt
