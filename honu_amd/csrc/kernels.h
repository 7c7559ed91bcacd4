// kernels.h — launch wrappers shared between the kernel translation units and
// the C ABI (api.hip). Every wrapper is asynchronous on `stream` and returns a
// hipError_t from the launch.
#pragma once

#include "common.h"
#include "lookback.h"

namespace honu {

// Per-record scratch handed from honu_decode_parse to honu_decode_fill.
struct DecodeScratch {
    uint64_t acl_pos;     // absolute offset of the first ACL entry flag
    uint64_t regions_pos; // absolute offset of the first region varint
    uint64_t data_src;    // absolute offset of the payload (Data() subslice)
    uint64_t rec_end;     // absolute end of the record
};

// Flag bits on DecodeScratch::acl_pos / regions_pos, set by the lane and group
// parses for the group fill (positions are < 2^62).
#define GRP_ACL_FAST (1ull << 63)    // acl_pos: every entry present, entry j at acl_pos + 18 j
#define GRP_REG_INLINE (1ull << 62)  // regions_pos: region ids in reg_inline[8 i ..]
// acl_pos bits 56-59 (GRP_ACL_FAST lists, HONU_GATHER_SKIP_WIN): how many of
// the list's first flags the walk already checked from its window (win.h)
#define GRP_ACL_A0_SHIFT 56
#define GRP_ACL_A0(pos) (((pos) >> GRP_ACL_A0_SHIFT) & 15ull)
// bits 53-55 (HONU_GATHER_SKIP_WIN2): how many of its last flags it checked
// from the window after the list
#define GRP_ACL_TL_SHIFT 53
#define GRP_ACL_TL(pos) (((pos) >> GRP_ACL_TL_SHIFT) & 7ull)
#define GRP_POS_MASK ((1ull << GRP_ACL_TL_SHIFT) - 1)  // positions < 2^53
// Flag on the lane encoder's ACL list position: every entry present, and the
// list's partial end chunks are already written (the group kernel stores the
// whole chunks in between).
#define ACL_ALL_PRESENT (1ull << 63)
// The memory side's write unit: a 64-byte unit that leaves L2 partly written
// costs a read-modify-write (tools/partial_write_probe.hip). The units form of
// the encode (honu_encode_*_units): the encoder writes a payload's partial end
// units, the copy the whole ones (lane.h encode_record_lane, copy.hip
// EncodeSegments).
#define PAYLOAD_UNIT 64ull

// 01 | ClientID | Permissions, the 18 encoded bytes of a present
// *AccessControl (acls.go:26-39), as 4.5 little-endian words.
HONU_DEV void acl_enc_words(const honu_acl *e, uint32_t d[5]) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(e);
    const uint32_t e0 = w[0], e1 = w[1], e2 = w[2], e3 = w[3], e4 = w[4];
    d[0] = 1u | (e0 << 8);
    d[1] = (e0 >> 24) | (e1 << 8);
    d[2] = (e1 >> 24) | (e2 << 8);
    d[3] = (e2 >> 24) | (e3 << 8);
    d[4] = (e3 >> 24) | ((e4 & 0xFF) << 8);
}

// 16 output bytes at absolute X >= P of the list at P (every entry present)
HONU_DEV u32x4 acl_chunk(const honu_acl *A, uint64_t na, uint64_t P, uint64_t X) {
    const uint64_t j0 = (X - P) / 18;
    uint32_t b[10];
    acl_enc_words(A + j0, b);
    b[5] = b[6] = b[7] = b[8] = b[9] = 0;
    if (j0 + 1 < na) {  // entry j0 + 1 starts at byte 18 of b
        uint32_t d[5];
        acl_enc_words(A + j0 + 1, d);
        b[4] = (b[4] & 0xFFFF) | (d[0] << 16);
        b[5] = (d[0] >> 16) | (d[1] << 16);
        b[6] = (d[1] >> 16) | (d[2] << 16);
        b[7] = (d[2] >> 16) | (d[3] << 16);
        b[8] = (d[3] >> 16) | (d[4] << 16);
    }
    // chunk byte k = byte (X - P - 18 j0) + k of b (X >= P)
    const uint32_t off = (uint32_t)(X - (P + 18 * j0));
    const uint32_t q = off >> 2, sh = off & 3;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t w0 = b[k], w1 = b[k + 1];
#pragma unroll
        for (int t = 1; t <= 4; t++)
            if ((uint32_t)t == q) {
                w0 = b[t + k];
                w1 = b[t + k + 1];
            }
        o[k] = __builtin_amdgcn_alignbyte(w1, w0, sh);
    }
    return u32x4{o[0], o[1], o[2], o[3]};
}

struct LaunchGeom {
    int num_cu;
    int per_record_blocks;  // cap on blocks for one-wave-per-record kernels
    int lane_blocks;        // cap on blocks for the lane / group / window kernels
                            // (0: one block per 256 lanes of work, no cap)
    int copy_blocks;        // blocks of the byte-balanced copy kernel
    int record_variant;     // per-record kernels: 0 auto (the fastest measured form
                            // of each; honu_decode_batch single-launch from 48 K
                            // records), 5 split decode, 6 single-launch decode
                            // at every size
    int seek_variant;       // honu_key_seek: 0 auto (by the probe and row counts), 1 the direct
                            // binary search, 2 the fenced one (seek.hip)
    uint32_t *copy_tickets; // the copies' range-tail counters (copy.hip): in the context's
                            // geometry the ring's first line, in a launch's copy its own line
    int copy_steal;         // 1: range tails from the counters (default), 0: off
};
#define COPY_TICKET_STRIDE 32u  // uint32 words: one 128-byte line per copy launch
#define COPY_TICKET_LINES 64u   // the ring: copy calls in flight at once on one context

hipError_t launch_encode_copy(const LaunchGeom &g, const uint8_t *payload,
                              const uint64_t *payload_off, uint64_t n, uint8_t *out,
                              uint64_t out_cap, const uint64_t *out_off, const int32_t *status,
                              bool units, hipStream_t s);

hipError_t launch_decode_copy(const LaunchGeom &g, const uint8_t *rec, uint64_t n,
                              const honu_record_info *info, const DecodeScratch *scratch,
                              const uint64_t *offs, const uint64_t *totals, uint8_t *data,
                              hipStream_t s);
hipError_t launch_decode_keys(const LaunchGeom &g, const honu_meta *meta,
                              const honu_record_info *info, uint64_t n, uint8_t *keys,
                              int32_t *key_status, hipStream_t s);

// The lane encoder's hand-over to the ACL list kernel, one per record: where
// the list goes (| ACL_ALL_PRESENT) and the row fields the list kernel needs,
// so that it reads 32 bytes per record instead of two lines of the row.
struct EncAclPos {
    uint64_t pos;        // the list's first byte in the output (| ACL_ALL_PRESENT)
    uint64_t acl_off;    // the row's acl_off / acl_count
    uint64_t acl_count;
    uint64_t carried;    // the row's acl_bytes | ENC_ACL_SIZED when HONU_ACL_SIZED is set
};
#define ENC_ACL_SIZED (1ull << 63)

// acl_out != null: the ACL entries are left out (hand-over in acl_out) for
// launch_encode_acl_grp
hipError_t launch_encode_meta_lane(const honu_meta *meta, const uint8_t *var, const honu_acl *acl,
                                   const uint32_t *reg, const uint64_t *payload_off, uint64_t n,
                                   uint8_t *out, uint64_t out_cap, const uint64_t *out_off,
                                   int32_t *status, EncAclPos *acl_out, int max_blocks, int num_cu,
                                   const uint8_t *payload, hipStream_t s);
hipError_t launch_encode_acl_grp(const honu_meta *meta, const honu_acl *acl, uint64_t n,
                                 uint8_t *out, int32_t *status, const EncAclPos *acl_pos,
                                 int max_blocks, hipStream_t s);
// the same with the lists placed by the kernel itself (no acl_pos), so that it
// can run beside launch_encode_meta_lane
hipError_t launch_encode_acl_grp_self(const honu_meta *meta, const honu_acl *acl, const uint64_t *payload_off,
                                      uint64_t n, uint8_t *out, uint64_t out_cap, const uint64_t *out_off,
                                      int32_t *status, int max_blocks, hipStream_t s);

hipError_t launch_encode_sizes_grp(const honu_meta *meta, uint64_t var_len, const honu_acl *acl,
                                   uint64_t acl_len, const uint32_t *reg, uint64_t reg_len,
                                   const uint64_t *payload_off, uint64_t n, uint64_t *sizes,
                                   int32_t *status, int max_blocks, hipStream_t s);
hipError_t launch_decode_fill_grp(const uint8_t *rec, uint64_t n, honu_meta *meta,
                                  honu_record_info *info, const DecodeScratch *scratch,
                                  const uint32_t *reg_inline, const uint64_t *counts,
                                  const uint64_t *offs, honu_acl *acl, uint64_t acl_cap,
                                  uint32_t *reg, uint64_t reg_cap, uint8_t *data,
                                  uint64_t data_cap, int max_blocks, hipStream_t s);

// fused.hip: one launch from records to rows, record info and tables
// (materialize: also the data-arena offsets honu_decode_payloads copies to)
int decode_walk_flag_checks();  // fused.hip: bit 0 window 1's flags, bit 1 window 2's
struct DecodeOut {
    honu_meta *meta;
    honu_record_info *info;
    honu_acl *acl;
    uint64_t acl_cap;
    uint32_t *reg;
    uint64_t reg_cap;
    uint64_t data_cap;
    int materialize;          // data offsets into a data arena (else zero-copy)
    DecodeScratch *scratch;   // materialize: payload sources for honu_decode_payloads
    uint64_t *offs;           // materialize: offs[3i+2] = data arena offset
    uint64_t *totals;         // column totals (3)
    bool reg_inplace;         // region lists returned in place (HONU_REGIONS_INPLACE)
};
// The context's look-back state of the launch (lookback.h): the ticket/epoch
// block, 3 status words per 64-record tile, then 3 per 64-tile group (words:
// both), and the pinned host words the guarded launch writes.
struct FusedState {
    LbState *lb;
    uint64_t *status, *gstatus;
    uint64_t words;
    uint32_t *spec_seen;  // [0] the back-off flag, [1] recoveries (a count)
};
struct FusedOpts {
    int max_blocks;    // cap on the launch's workgroups (0: none)
    int guard_blocks;  // one-wave workgroups of the guarded launch (0: as many as the launch has waves)
    bool speculate;    // launches of FUSED_SPEC_MIN_TILES tiles and more speculate
    bool acl_inplace;  // all-present ACL lists returned in place (HONU_ACL_INPLACE)
};
hipError_t launch_decode_fused(const uint8_t *rec, const uint64_t *rec_off, uint64_t n,
                               const DecodeOut &O, const FusedState &F, const FusedOpts &opt, hipStream_t s);

hipError_t launch_decode_parse_win(const uint8_t *rec, const uint64_t *rec_off, uint64_t n,
                                   honu_meta *meta, honu_record_info *info,
                                   DecodeScratch *scratch, uint32_t *reg_inline, uint64_t *counts,
                                   int max_blocks, bool inplace, bool reg_inplace, hipStream_t s);

hipError_t launch_system_sizes(const honu_collection *rows, uint64_t var_len, const honu_acl *acl,
                               uint64_t acl_len, const uint32_t *reg, uint64_t reg_len,
                               const honu_index *idx, uint64_t idx_len, uint64_t n,
                               uint64_t *sizes, int32_t *status, hipStream_t s);
hipError_t launch_system_encode(const honu_collection *rows, const uint8_t *var,
                                const honu_acl *acl, const uint32_t *reg, const honu_index *idx,
                                uint64_t n, uint8_t *out, uint64_t out_cap,
                                const uint64_t *out_off, int32_t *status, hipStream_t s);
hipError_t launch_system_parse(const uint8_t *rec, const uint64_t *rec_off, uint64_t n,
                               bool headless, honu_collection *rows, int32_t *status,
                               DecodeScratch *scratch, uint64_t *counts, hipStream_t s);
hipError_t launch_system_fill(const uint8_t *rec, uint64_t n, honu_collection *rows,
                              int32_t *status, const DecodeScratch *scratch,
                              const uint64_t *counts, const uint64_t *offs, honu_acl *acl,
                              uint64_t acl_cap, uint32_t *reg, uint64_t reg_cap, honu_index *idx,
                              uint64_t idx_cap, hipStream_t s);

hipError_t launch_decode_headers(const uint8_t *rec, const uint64_t *rec_off, uint64_t n,
                                 honu_record_info *info, hipStream_t s);
hipError_t launch_decode_spans(const uint8_t *rec, const uint64_t *rec_off, uint64_t n,
                               honu_record_info *info, DecodeScratch *scratch, uint64_t *counts,
                               hipStream_t s);
hipError_t launch_decode_data_place(uint64_t n, honu_record_info *info, const uint64_t *offs,
                                    uint64_t data_cap, hipStream_t s);
hipError_t launch_span_copy(const LaunchGeom &g, const uint8_t *rec, uint64_t n,
                            const honu_record_info *info, const DecodeScratch *scratch,
                            const uint64_t *offs, uint8_t *data, hipStream_t s);

// Exclusive scan of K interleaved u64 columns: out[i*K+c] = sum_{j<i} in[j*K+c];
// totals[c] = full sum. One launch (decoupled look-back over tiles); the
// state is the context's (scan_status_words(n) status words).
struct ScanState {
    LbState *lb;
    uint64_t *status;
    uint64_t words;
    int max_blocks;
};
uint64_t scan_status_words(uint64_t n);
hipError_t launch_scan(const uint64_t *in, uint64_t n, int K, uint64_t *out, uint64_t *totals,
                       const ScanState &S, hipStream_t s);

// a workspace's parts start on 256-byte boundaries
inline uint64_t up256(uint64_t x) { return (x + 255) & ~255ull; }

// sort.hip: sort.Sort(keys.Keys) (keys.go:126-130) and the objects' version
// ranges (keys.go:73-92). The caller's workspace, carved: the plan words, the
// two sides of packed keys (32 bytes each) and indices, the one scan column
// (n + 1 rows) and the digit-major count table (256 rows per tile).
struct SortWork {
    uint32_t *plan;
    u32x4 *key[2];
    uint32_t *idx[2];
    uint64_t *col;
    uint64_t *table;
};
uint32_t sort_tile();
uint64_t sort_workspace_bytes(uint64_t n);
SortWork sort_carve(void *work, uint64_t n);
// scan_rows: the rows the context's scan state covers (its max_records)
hipError_t launch_sort_keys(const uint8_t *keys, const int32_t *status, uint64_t n, uint32_t *order,
                            uint8_t *sorted, uint64_t *valid, void *work, const ScanState &S,
                            uint64_t scan_rows, hipStream_t s);
hipError_t launch_key_objects(const uint8_t *keys, const uint32_t *order, const uint64_t *valid, uint64_t n,
                              uint64_t *obj_off, uint32_t *latest, uint64_t *objects, void *work,
                              const ScanState &S, hipStream_t s);

// seek.hip: Cursor.Seek (iterator/cursor.go:44-55) for a batch of probes over
// the sorted column. variant: 0 auto, 1 direct, 2 fenced (LaunchGeom::seek_variant)
uint32_t seek_fence();
uint64_t seek_auto_probes();  // variant 0 takes the direct form for fewer probes than this ...
uint64_t seek_auto_keys();    // ... over more rows than this, the fenced form otherwise
hipError_t launch_key_seek(int variant, int num_cu, const uint8_t *sorted, const uint64_t *valid, uint64_t n,
                           const uint8_t *probes, const int32_t *pstatus, uint32_t probe_len, uint64_t m,
                           const uint32_t *order, const honu_record_info *info, honu_seek *out, hipStream_t s);

// merge.hip: a batch of Puts (store.go:232, 395, 530) into the sorted column: the stable
// merge of two of launch_sort_keys' outputs, A first on equal keys. na + nb <= 2^32 - 1;
// order == null merges the column alone
uint32_t merge_tile();
hipError_t launch_key_merge(const uint8_t *sa, const uint32_t *oa, const uint64_t *valid_a, uint64_t na,
                            const uint8_t *sb, const uint32_t *ob, const uint64_t *valid_b, uint64_t nb,
                            uint32_t b_base, uint8_t *out, uint32_t *order, uint64_t *valid_out, hipStream_t s);

// delete.hip: a batch of Deletes (store.go:378-383, 399-404) from the sorted column and the rows
// a Put superseded: a stable compaction, kept rows, removed rows, the invalid tail. n, m <=
// 2^32 - 1; order_out == null compacts the column alone; removed may be null. The workspace is
// the caller's (delete_workspace_bytes(n)). The tiles' counts go through launch_scan: delete_tiles(n)
// must not exceed the rows the context's scan state covers (its max_records)
uint32_t delete_tile();
uint64_t delete_tiles(uint64_t n);
uint64_t delete_workspace_bytes(uint64_t n);
hipError_t launch_key_delete(const uint8_t *sorted, const uint32_t *order, const uint64_t *valid, uint64_t n,
                             const uint8_t *del, const uint64_t *valid_del, uint64_t m, uint32_t probe_len,
                             uint32_t flags, uint8_t *out, uint32_t *order_out, uint64_t *valid_out,
                             uint64_t *removed, void *work, const ScanState &S, hipStream_t s);

// list.hip: a batch of cursor walks (Next / Prev, iterator/cursor.go:57-89) over ranges of the sorted
// column, honu_key_seek's rows: the rows each would visit, packed, the ranges in order. n, m, cap <=
// 2^32 - 1. No workspace; the counts are scanned in place in range_off (m + 1 values) through
// launch_scan: m + 1 must not exceed the rows the context's scan state covers (its max_records)
uint32_t list_tile();
uint32_t list_stage();
hipError_t launch_key_list(int num_cu, const uint8_t *sorted, const uint32_t *order, const uint64_t *valid, uint64_t n,
                           const honu_seek *ranges, uint64_t m, uint32_t limit, uint32_t flags,
                           const uint64_t *obj_off, const uint64_t *objects, const honu_record_info *info,
                           uint64_t *range_off, honu_list_row *rows, uint8_t *keys_out, uint64_t cap,
                           uint64_t *total, const ScanState &S, hipStream_t s);

// fetch.hip: Cursor.Object() (iterator/cursor.go:31-38) for the rows of a list: the records they name,
// packed into a CSR arena (val_off: cap + 1 values, the lengths scanned in place through launch_scan, so
// cap + 1 must not exceed the rows the context's scan state covers). cap, nrec <= 2^32 - 1. No workspace.
// g: the call's own copy geometry (api.hip copy_geom). The copy itself is launch_fetch_copy (copy.hip),
// FetchSegments over the byte-balanced engine
hipError_t launch_key_fetch(const LaunchGeom &g, const honu_list_row *rows, const uint64_t *total, uint64_t cap,
                            const uint8_t *rec, const uint64_t *rec_off, uint64_t nrec, uint64_t rec_bytes,
                            uint32_t flags, uint64_t *val_off, int32_t *status, uint8_t *values, uint64_t val_cap,
                            uint64_t *val_total, const ScanState &S, hipStream_t s);
hipError_t launch_fetch_copy(const LaunchGeom &g, const honu_list_row *rows, uint64_t n, const uint8_t *rec,
                             const uint64_t *rec_off, const uint64_t *val_off, uint8_t *values,
                             uint64_t val_cap, hipStream_t s);

// filter.hip: the live-object filter (collection.go:132-134) over the rows of a list: a stable compaction
// of the rows (and their keys) that stay, the ranges' offsets and HEAD flags recomputed. m, cap, n <=
// 2^32 - 1. The workspace is the caller's (filter_workspace_bytes(cap)). The tiles' counts go through
// launch_scan: filter_tiles(cap) must not exceed the rows the context's scan state covers (its max_records).
// The column's arrays (valid .. info) are read with HONU_FILTER_DELETED only
uint32_t filter_tile();
uint64_t filter_tiles(uint64_t cap);
uint64_t filter_workspace_bytes(uint64_t cap);
hipError_t launch_key_filter(const honu_list_row *rows, const uint8_t *keys, const uint64_t *range_off, uint64_t m,
                             const uint64_t *total, uint64_t cap, uint32_t flags, const uint64_t *valid, uint64_t n,
                             const uint64_t *obj_off, const uint32_t *latest, const uint64_t *objects,
                             const honu_record_info *info, honu_list_row *rows_out, uint8_t *keys_out,
                             uint64_t *range_off_out, uint64_t *total_out, void *work, const ScanState &S,
                             hipStream_t s);

// next.hip: the version each of a batch of writes writes (lamport/pid.go:10-15; collection.go:75-137;
// store.go:361-395): requests are 17-byte object prefixes in 29-byte rows, ranked among themselves through
// launch_sort_keys and looked up in the resident column as honu_key_seek's 17-byte probes. n, m <= 2^32 - 1; m
// must not exceed scan_rows, the rows the context's scan state covers (its max_records). The workspace is the
// caller's (next_workspace_bytes(m)); order, info, rstatus and meta may be null
uint64_t next_workspace_bytes(uint64_t m);
hipError_t launch_key_next(const uint8_t *sorted, const uint64_t *valid, uint64_t n, const uint32_t *order,
                           const honu_record_info *info, const uint8_t *req, const int32_t *rstatus, uint64_t m,
                           uint32_t op, uint32_t pid, uint32_t region, int64_t now, honu_next *out, uint8_t *keys_out,
                           int32_t *key_status, honu_meta *meta, void *work, const ScanState &S, uint64_t scan_rows,
                           hipStream_t s);

// compare.hip: the versions of two sorted columns compared object by object (lamport/scalar.go:15-78;
// keys/keys.go:35-36): per object of A (obj_off, objects: launch_key_objects') one honu_seek row, the rows the
// peer B is behind by and the HONU_CMP_* class. na, nb <= 2^32 - 1. The workspace is the caller's
// (compare_workspace_bytes(na)); no scan state. stage: the rows of B a workgroup stages at most (compare_stage()
// and no more); order_a, peer and counts may be null
uint32_t compare_tile();
uint32_t compare_stage();
uint64_t compare_workspace_bytes(uint64_t na);
hipError_t launch_key_compare(const uint8_t *sa, const uint32_t *order_a, const uint64_t *valid_a, uint64_t na,
                              const uint64_t *obj_off, const uint64_t *objects, const uint8_t *sb,
                              const uint64_t *valid_b, uint64_t nb, uint32_t stage, honu_seek *out, uint32_t *peer,
                              uint64_t *counts, void *work, hipStream_t s);

// reclaim.hip: the space a Drop frees (store.go:314-322, 399-404): the records a valid row of the column names,
// renumbered in ascending old index, with their per-record arrays (keys, key_status, info: each null or given with
// its output) and their bytes packed into a new CSR arena (rec_off_out: nrec + 1 values, the lengths scanned in
// place through launch_scan, so nrec + 1 must not exceed the rows the context's scan state covers). n, nrec <=
// 2^32 - 1. The workspace is the caller's (reclaim_workspace_bytes(nrec)); remap and status may be null. g: the
// call's own copy geometry. The copy itself is launch_reclaim_copy (copy.hip), ReclaimSegments over the
// byte-balanced engine
uint32_t reclaim_tile();
uint64_t reclaim_workspace_bytes(uint64_t nrec);
hipError_t launch_key_reclaim(const LaunchGeom &g, const uint32_t *order, const uint64_t *valid, uint64_t n,
                              const uint8_t *keys, const int32_t *key_status, const honu_record_info *info,
                              const uint8_t *rec, const uint64_t *rec_off, uint64_t nrec, uint64_t rec_bytes,
                              uint32_t *order_out, uint32_t *remap, uint32_t *source, uint8_t *keys_out,
                              int32_t *key_status_out, honu_record_info *info_out, uint64_t *rec_off_out,
                              int32_t *status, uint8_t *values, uint64_t val_cap, uint64_t *kept,
                              uint64_t *val_total, void *work, const ScanState &S, hipStream_t s);
hipError_t launch_reclaim_copy(const LaunchGeom &g, const uint32_t *source, uint64_t n, const uint8_t *rec,
                               const uint64_t *rec_off, const uint64_t *val_off, uint8_t *values,
                               uint64_t val_cap, hipStream_t s);

// route.hip: a batch taken apart by collection, the bucket of every write (store.go:236-240; tx.go:112-120, 141-158;
// collection.go:86): per position its class in the table of collections (k rows of 16 bytes, ascending; route_find.h),
// then the stable partition of the positions by class through launch_sort_keys over the packed classes, so m must not
// exceed scan_rows, the rows the context's scan state covers (its max_records). m <= 2^32 - 1, k <= 2^32 - 4. The
// workspace is the caller's (route_workspace_bytes(m)); status, seq, keys with keys_out, bucket, rows and local may be
// null. route_stage(): the table rows a workgroup stages in LDS at most
uint32_t route_stage();
uint64_t route_workspace_bytes(uint64_t m);
hipError_t launch_key_route(const uint8_t *ids, uint64_t id_stride, const int32_t *status, uint64_t m,
                            const uint32_t *seq, const uint8_t *table, uint64_t k, const uint8_t *keys,
                            uint32_t *bucket, honu_list_row *rows, uint32_t *local, uint8_t *keys_out,
                            uint64_t *bucket_off, uint64_t *bucket_count, void *work, const ScanState &S,
                            uint64_t scan_rows, hipStream_t s);

// merge_buckets.hip: a routed batch merged into every bucket's column at once (store.go:232-240, 395, 530; tx.go:112-120):
// two bucketed columns (k buckets end to end in one arena, offsets k + 1 values; bucket_off.h), per bucket the stable
// merge of its valid A rows and its B rows, the buckets tight behind each other. na + nb <= 2^32 - 1, k <= 2^32 - 4; oa,
// count_a, ob, base, order and count_out may be null. With count_a the buckets' rows go through launch_scan in off_out
// (k values, the total to off_out[k]): k must not exceed the rows the context's scan state covers (its max_records).
// merge_buckets_stage(): the buckets a tile touches at most for its slice of offsets to be staged in LDS
uint32_t merge_buckets_stage();
hipError_t launch_merge_buckets(uint64_t k, const uint8_t *sa, const uint32_t *oa, const uint64_t *off_a,
                                const uint64_t *count_a, uint64_t na, const uint8_t *sb, const uint32_t *ob,
                                const uint64_t *off_b, uint64_t nb, const uint32_t *base, uint32_t b_base, uint8_t *out,
                                uint32_t *order, uint64_t *off_out, uint64_t *count_out, const ScanState &S,
                                hipStream_t s);

hipError_t launch_hbm_probe(int mode, const void *src, void *dst, uint64_t bytes, uint32_t blocks,
                            uint32_t *sink, hipStream_t s);
hipError_t launch_gen_payload(const LaunchGeom &g, uint64_t seed, uint64_t first, uint64_t n,
                              const uint64_t *payload_off, uint8_t *payload, hipStream_t s);
hipError_t launch_verify_decoded(const LaunchGeom &g, const honu_meta *src, const uint8_t *var,
                                 const honu_acl *src_acl, const uint32_t *src_reg,
                                 const uint64_t *payload_off, const uint8_t *rec,
                                 const honu_meta *dec, const honu_record_info *info,
                                 const honu_acl *dec_acl, const uint32_t *dec_reg, uint64_t n,
                                 uint32_t *mismatch, hipStream_t s);
hipError_t launch_digest(const LaunchGeom &g, const uint8_t *arena, const uint64_t *off,
                         const uint64_t *len, uint64_t n, uint64_t *digest, hipStream_t s);

}  // namespace honu
