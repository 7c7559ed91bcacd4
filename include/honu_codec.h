/*
 * honu_codec.h — C ABI of the MI355X-native batch object-record codec.
 *
 * This is the drop-in boundary for Honu's reflection-free object codec
 * (rotationalio/honu, pkg/store/object + pkg/store/lani + pkg/store/metadata).
 * The reference has no FFI at all (it is pure Go, CGO_ENABLED=0); the entry
 * points below are what a cgo shim behind a `honu_hip` build tag binds so that
 * pkg/store keeps its Go API (see INTEGRATION.md for the cgo stub).
 *
 *   reference (Go, one record per call)               this ABI (one batch per call)
 *   -----------------------------------------------   ------------------------------------------
 *   object.Marshal(meta, data)  object.go:24-45        honu_encode_sizes + honu_exclusive_scan
 *                                                       + honu_encode   (or honu_marshal_batch)
 *   Object.Metadata()           object.go:66-83        honu_decode_parse + honu_decode_fill
 *   Object.Data()               object.go:85-99          (or honu_decode_batch); per-record
 *   Object.Tombstone()          object.go:103-112        results land in honu_record_info
 *   Object.StorageVersion()     object.go:47-52
 *   Object.Key()                object.go:57-64        honu_decode_keys (29-byte keys.Key column)
 *   sort.Sort(keys.Keys)        keys/keys.go:126-130   honu_sort_keys (stable order of the column)
 *   an object's versions        keys/keys.go:73-92     honu_key_objects (ranges of the order, latest)
 *   Cursor.Seek, Has, Exists    iterator/cursor.go:44-55  honu_key_seek (positions of a batch of probes)
 *   bucket.Put (a batch)        store.go:232, 395, 530 honu_key_merge (stable merge into the sorted column)
 *   bucket.Delete (a batch)     store.go:378-383, 399-404 honu_key_delete (stable compaction of the sorted column)
 *   Cursor.Next / Prev (batch)  iterator/cursor.go:57-89  honu_key_list (the rows of a batch of seek ranges, packed)
 *   Cursor.Object() (batch)     iterator/cursor.go:31-38  honu_key_fetch (the records the listed rows name, a CSR arena)
 *   deleted objects not listed  collection.go:132-134, 97-101  honu_key_filter (stable compaction of the listed rows)
 *   pid.Next, Tombstone (batch) lamport/pid.go:10-15, collection.go:75-137  honu_key_next (the version each write writes)
 *   lamport.Compare (two columns) lamport/scalar.go:15-78, keys/keys.go:35-36  honu_key_compare (who is later, what to send, forks)
 *   Drop "to free up space"     store.go:314-322, 399-404  honu_key_reclaim (the records arena compacted to the records the column names)
 *   tx.Bucket(collectionID[:])  store.go:236-240, tx.go:112-120, 141-158  honu_key_route (a mixed batch partitioned by its collections' buckets)
 *   bucket.Put (every bucket)   store.go:232-240, 395, 530, tx.go:112-120  honu_key_merge_buckets (a routed batch merged into all buckets' columns)
 *   lani.Encodable.Size()       lani/lani.go:9-12     (host only; Size() is a Grow hint, not bytes)
 *
 * Conventions
 *   - Every pointer argument named d_* is DEVICE memory (hipMalloc / torch
 *     tensor storage) unless stated; every call is asynchronous on `stream`
 *     (a hipStream_t passed as void*, NULL = the null stream). No call
 *     allocates, frees or synchronises, so a sequence of calls can be
 *     captured into a hipGraph.
 *   - Batches are CSR: record i occupies bytes [off[i], off[i+1]) of an arena.
 *   - Functions return an honu_status for argument errors (HONU_E_ARG,
 *     HONU_E_WORKSPACE, HONU_E_HIP); per-record outcomes are written to device
 *     status arrays using the same enum.
 *   - The library is gfx950-only; it fails loudly (HONU_E_NO_DEVICE) when no
 *     gfx950 device is present. There is no CPU fallback.
 *   - What a call stores, to the byte: the ranges [off[i], off[i+1]) of the
 *     records it completes (status HONU_OK after the call); the first n rows,
 *     infos, sizes / offsets (n + 1 where stated) and statuses; the table
 *     entries of the records that fit their table; the payload ranges
 *     [data_off, data_off + data_len) it reports with data_status HONU_OK;
 *     and its totals (3 x u64 = 24 bytes, 8 for honu_decode_data). It never
 *     stores in the range of a record that failed or that it was told to skip
 *     (a status other than HONU_OK on entry), at or past a capacity (out_cap,
 *     acl_cap, regions_cap, data_cap: a record or payload that does not fit
 *     is not stored in part), in the data arena's 16-byte alignment gaps or
 *     behind its last payload, in a neighbouring record's bytes of a shared
 *     16- or 64-byte chunk, or anywhere before or behind a buffer. The
 *     encode calls, honu_marshal_batch, honu_decode_batch and
 *     honu_exclusive_scan check their arguments (the alignments stated at
 *     honu_ctx_create, n against max_records) before their first launch:
 *     refused with HONU_E_ARG or HONU_E_WORKSPACE, they have stored nothing.
 *     Outputs may therefore lie back to back with memory the caller still
 *     uses, and a result does not depend on where an arena lies.
 */
#ifndef HONU_CODEC_H
#define HONU_CODEC_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HONU_ABI_VERSION 6u  /* 6: region lists returned in place (HONU_REGIONS_INPLACE);
                                5: honu_encode_*_units; 4: ACL lists returned in place (HONU_ACL_INPLACE) */
#define HONU_STORAGE_VERSION 1u /* object.StorageVersion, object.go:14 */
#define HONU_ULID_LEN 16
#define HONU_KEY_LEN 29         /* keys.keySize, keys/keys.go:14 */

/* ------------------------------------------------------------------------ */
/* Status codes. Per-record codes map 1:1 to the Go sentinels.              */
/* ------------------------------------------------------------------------ */
typedef enum honu_status {
    HONU_OK = 0,
    HONU_ERR_BAD_VERSION = 1,    /* object.ErrBadVersion     object/errors.go:6 */
    HONU_ERR_MALFORMED = 2,      /* object.ErrMalformed      object/errors.go:7 */
    HONU_ERR_EOF = 3,            /* io.EOF                   lani/decode.go:95,129,151,173,195,211 */
    HONU_ERR_UNEXPECTED_EOF = 4, /* io.ErrUnexpectedEOF      lani/decode.go:47,200,215 */
    HONU_ERR_NO_LENGTH = 5,      /* lani.ErrNoLength         lani/errors.go:8 */
    HONU_ERR_PARSE_BOOLEAN = 6,  /* lani.ErrParseBoolean     lani/errors.go:9 */
    HONU_ERR_PARSE_VARINT = 7,   /* lani.ErrParseVarInt      lani/errors.go:10 */
    HONU_ERR_PANIC = 8,          /* input on which the Go reference panics (slice
                                    out of range object.go:77,97; makeslice
                                    decode.go:50, metadata.go:255, region.go:160;
                                    nil *Metadata in Marshal metadata.go:66) */
    HONU_ERR_CAPACITY = 9,       /* an output arena/table was too small (ABI only) */
    HONU_ERR_INPUT = 10,         /* an encode input span/list points outside its arena (ABI only) */
    HONU_UNPARSED = 11,          /* meta_status of honu_decode_headers: Metadata() not evaluated */
    /* call-level errors (returned, never written per record) */
    HONU_E_ARG = -1,
    HONU_E_WORKSPACE = -2,       /* n exceeds the context's reserved record count */
    HONU_E_HIP = -3,             /* a HIP runtime call failed */
    HONU_E_NO_DEVICE = -4        /* no gfx950 device / kernels not loadable */
} honu_status;

/* ------------------------------------------------------------------------ */
/* Data layout                                                               */
/* ------------------------------------------------------------------------ */

/* A byte range inside an arena. Zero length == nil == empty: lani frames of
 * length 0 decode to nil (lani/decode.go:37-39) and nil/empty encode alike. */
typedef struct honu_span {
    uint64_t off;
    uint64_t len;
} honu_span;

/* Presence bits of honu_meta.present (the lani nil-flag bytes). */
enum {
    HONU_HAS_META = 1u << 0,        /* object-level Metadata nil flag (object.go:40) */
    HONU_HAS_VERSION = 1u << 1,     /* Metadata.Version      metadata.go:20 */
    HONU_HAS_PARENT = 1u << 2,      /* Version.Parent        version.go:17 */
    HONU_HAS_SCHEMA = 1u << 3,      /* Metadata.Schema       metadata.go:21 */
    HONU_HAS_PUBLISHER = 1u << 4,   /* Metadata.Publisher    metadata.go:28 */
    HONU_HAS_ENCRYPTION = 1u << 5,  /* Metadata.Encryption   metadata.go:29 */
    HONU_HAS_COMPRESSION = 1u << 6, /* Metadata.Compression  metadata.go:30 */
    HONU_REGIONS_NONNIL = 1u << 7,  /* set by decode: Regions.Decode always makes a
                                       (possibly empty) slice, region.go:160 */
    HONU_ACL_INPLACE = 1u << 8,     /* set by decode (honu_meta only): the ACL list is
                                       returned in place, see honu_meta.acl_off */
    HONU_REGIONS_INPLACE = 1u << 9, /* set by decode (honu_meta only): the region list
                                       is returned in place, see honu_meta.regions_off */
    HONU_ACL_SIZED = 1u << 10       /* encode input (honu_meta only): acl_bytes holds the
                                       ACL list's encoded length, see honu_meta.acl_bytes */
};

/* One metadata.Metadata (metadata.go:17-35) flattened into a fixed 352-byte
 * row. Rows are the encode input and the decode output.
 *   encode: spans index `var_arena`, acl_off/acl_count index the ACL table,
 *           regions_off/regions_count index the region table.
 *   decode: spans are ABSOLUTE offsets into the records arena (zero copy, like
 *           lani.DecodeFixed), regions_off indexes the output region table.
 *           The ACL list comes back in one of two forms:
 *           - in place (HONU_ACL_INPLACE set in `present`; the default, context
 *             param "acl_inplace" 1): every entry of the list is present, and
 *             acl_off is the ABSOLUTE offset in the records arena of the first
 *             entry's encoding; entry j is the 18 bytes at acl_off + 18*j:
 *             0x01 | ClientID[16] | Permissions (acls.go:26-51), so
 *             ACL[j] = &AccessControl{rec[acl_off+18j+1 : +17], rec[acl_off+18j+17]};
 *           - table (HONU_ACL_INPLACE clear, acl_count > 0): a list holding a
 *             nil entry, or every list when "acl_inplace" is 0: acl_off indexes
 *             the honu_acl output table (present == 0 is a nil entry).
 *           Go copies every entry into a new *AccessControl either way
 *           (metadata.go:254-266); the in-place form leaves that copy to the
 *           binding, as Data() and the string spans already do.
 *           The region list likewise:
 *           - in place (HONU_REGIONS_INPLACE set; the default, context param
 *             "regions_inplace" 1, every non-empty list): regions_off is the
 *             ABSOLUTE offset in the records arena of the first region's
 *             uvarint; the regions_count uvarints follow back to back, each
 *             decoded as lani.DecodeUint32 does (at most 5 bytes, the value
 *             truncated to uint32: decode.go:127-146). The decode has already
 *             validated every one of them (a bad varint fails the record), so
 *             the binding's Regions.Decode loop (region.go:154-169) cannot fail;
 *           - table (HONU_REGIONS_INPLACE clear, regions_count > 0; every list
 *             when "regions_inplace" is 0): regions_off indexes the uint32
 *             output region table.
 *           In-place lists and spans point into the records arena: the row is
 *           valid while that arena is. Encode input rows must use the table
 *           forms: a row with HONU_ACL_INPLACE or HONU_REGIONS_INPLACE set gets
 *           HONU_ERR_INPUT from honu_encode_sizes.
 *   encode, HONU_ACL_SIZED (optional, what a binding's flatten sets while it
 *           copies m.ACL): acl_bytes = sum over the list of 18 per present
 *           entry and 1 per nil one (acls.go:26-39, encode.go:210-226), so the
 *           size pass reads no ACL table entry (the list kernel reads every
 *           entry anyway and checks the length: a row whose acl_bytes is not
 *           the list's length gets HONU_ERR_INPUT from the records call and
 *           its range of the output holds unspecified bytes; a value outside
 *           [acl_count, 18 * acl_count] is rejected by honu_encode_sizes).
 *           Without the bit the size pass reads the list from the table.
 * Times are Go UnixNano with 0 <=> time.Time{}.IsZero() (lani/encode.go:201-206,
 * decode.go:224-237). Fields of absent (nil) sub-structs are zero on decode. */
typedef struct honu_meta {
    uint32_t present;            /*   0 HONU_HAS_* bits */
    uint8_t permissions;         /*   4 Metadata.Permissions */
    uint8_t flags;               /*   5 Metadata.Flags */
    uint8_t tombstone;           /*   6 Version.Tombstone (bool, 0/1) */
    uint8_t compression_alg;     /*   7 Compression.Algorithm */
    uint8_t sealing_alg;         /*   8 Encryption.SealingAlgorithm */
    uint8_t encryption_alg;      /*   9 Encryption.EncryptionAlgorithm */
    uint8_t signature_alg;       /*  10 Encryption.SignatureAlgorithm */
    uint8_t _pad0;               /*  11 */
    uint32_t region;             /*  12 Version.Region */
    uint64_t vid;                /*  16 Version.Scalar.VID */
    uint32_t pid;                /*  24 Version.Scalar.PID */
    uint32_t parent_pid;         /*  28 Version.Parent.PID */
    uint64_t parent_vid;         /*  32 Version.Parent.VID */
    int64_t version_created;     /*  40 Version.Created */
    uint32_t schema_major;       /*  48 SchemaVersion.Major */
    uint32_t schema_minor;       /*  52 */
    uint32_t schema_patch;       /*  56 */
    uint32_t _pad1;              /*  60 */
    int64_t compression_level;   /*  64 Compression.Level */
    int64_t created;             /*  72 Metadata.Created */
    int64_t modified;            /*  80 Metadata.Modified */
    uint64_t acl_bytes;          /*  88 encode input with HONU_ACL_SIZED: the ACL
                                        list's encoded length; 0 on decode */
    uint8_t object_id[16];       /*  96 Metadata.ObjectID */
    uint8_t collection_id[16];   /* 112 Metadata.CollectionID */
    uint8_t owner[16];           /* 128 Metadata.Owner */
    uint8_t group[16];           /* 144 Metadata.Group */
    uint8_t publisher_id[16];    /* 160 Publisher.PublisherID */
    uint8_t client_id[16];       /* 176 Publisher.ClientID */
    honu_span schema_name;       /* 192 SchemaVersion.Name */
    honu_span mime;              /* 208 Metadata.MIME */
    honu_span ip_address;        /* 224 Publisher.IPAddress (net.IP bytes) */
    honu_span user_agent;        /* 240 Publisher.UserAgent */
    honu_span public_key_id;     /* 256 Encryption.PublicKeyID */
    honu_span encryption_key;    /* 272 Encryption.EncryptionKey */
    honu_span hmac_secret;       /* 288 Encryption.HMACSecret */
    honu_span signature;         /* 304 Encryption.Signature */
    uint64_t acl_off;            /* 320 first entry in the ACL table, or (decode,
                                        HONU_ACL_INPLACE) in the records arena */
    uint64_t acl_count;          /* 328 len(Metadata.ACL); 0 <=> nil */
    uint64_t regions_off;        /* 336 first entry in the region table, or (decode,
                                        HONU_REGIONS_INPLACE) in the records arena */
    uint64_t regions_count;      /* 344 len(Metadata.WriteRegions) */
} honu_meta;                     /* 352 */

/* One *metadata.AccessControl (acls.go:12-15); present==0 is a nil pointer
 * in the ACL slice (encoded as a single 0x00 flag byte). */
typedef struct honu_acl {
    uint8_t client_id[16];
    uint8_t permissions;
    uint8_t present;
    uint8_t _pad[2];
} honu_acl; /* 20 */

/* Per-record decode results: the Object methods object.go:47-112. */
typedef struct honu_record_info {
    uint64_t data_off;       /* payload: absolute offset in the records arena
                                (zero copy, like Data()'s subslice) or in the
                                data arena when materialising */
    uint64_t data_len;       /* len(Data()); 0 also for nil */
    int32_t data_status;     /* error of Object.Data() */
    int32_t meta_status;     /* error of Object.Metadata() */
    uint8_t storage_version; /* Object.StorageVersion() */
    uint8_t tombstone;       /* Object.Tombstone() */
    uint8_t _pad[6];
} honu_record_info; /* 32 */

/* ------------------------------------------------------------------------ */
/* Context                                                                   */
/* ------------------------------------------------------------------------ */
typedef struct honu_ctx honu_ctx;

/* Create a context on HIP device `device` with scratch for batches of up to
 * `max_records` records (scan partials, decode list positions). Allocation
 * happens here and only here. Returns NULL and sets *err on failure.
 * The scratch is per context: calls that use it (scans, decodes and the decode
 * payload copies, which read the decode's scratch) issued on different
 * streams concurrently need one context each. The encode payload copies
 * (honu_encode_payloads*) use none and may run concurrently on one context:
 * every copy call takes its own range-tail counter line from a ring of 64
 * (param "copy_steal"), so up to 64 copies may be in flight at once on one
 * context. The library reads no environment variable: a
 * context is configured through honu_ctx_set_param only. Arenas: the records
 * arena, the materialised data arena and row arrays must be 16-byte aligned,
 * ACL and region tables 4-byte aligned (hipMalloc gives 256). */
honu_ctx *honu_ctx_create(int device, uint64_t max_records, int32_t *err);
void honu_ctx_destroy(honu_ctx *ctx);
uint64_t honu_ctx_max_records(const honu_ctx *ctx);

/* The single-launch decode and the one-launch scans keep decoupled look-back
 * state in the context (a tile ticket, a finished-workgroup count and a launch
 * epoch) that each launch leaves clean for the next, so nothing is cleared
 * per call and the calls replay from a captured hipGraph. A launch that did
 * not run to completion (its stream was torn down, the device reset) can leave
 * it dirty: a context that saw a HIP error (HONU_E_HIP) must be reset with
 * honu_ctx_reset, on a stream with no other work of this context in flight,
 * before its next decode or scan (it returns when the reset is done). */
int32_t honu_ctx_reset(honu_ctx *ctx, void *stream);

/* Launch-geometry knobs (defaults suit MI355X): "copy_blocks" (workgroups of
 * the payload copy kernel, default 2 per CU), "record_blocks" (cap on
 * workgroups of the one-wave-per-record kernels, default 8 per CU),
 * "lane_blocks" (cap on workgroups of the lane, group and window kernels;
 * default 0 = no cap — a cap leaves room for a concurrent payload copy),
 * "copy_variant" (kept for compatibility: 0 only), "copy_steal" (1, the
 * default: in a copy whose payloads average >= 16 KB each streaming wave
 * copies 7/8 of its byte range, then the ranges' last eighths from a counter
 * in the context; 0: fixed ranges only), "record_variant" (how the
 * per-record metadata kernels map records to lanes: 0 auto — the fastest
 * measured form per kernel, with honu_decode_batch running the single-launch
 * decode for batches of 48 K records or more; 5 the split decode at every
 * size; 6 the single-launch decode at every size), "encode_variant" (kept for
 * compatibility: 0 only, one record per lane + the ACL lists by 16-lane
 * groups), "speculate" (the
 * single-launch decode's speculation, see honu_decode_records: 2 auto, the
 * default — only in materialising calls and the table forms, where it hides
 * look-back waits; 1 in every call; 0 off), "speculate_backoff" (0..16: the calls left without
 * speculation after a recovery; setting it also forgets a recovery the host
 * has not seen yet), "encode_fork" (honu_encode_records: 1 runs the ACL lists'
 * kernel, which then places the lists itself, on a stream of the context's own
 * beside the header/tail encoder, forked from and joined back into the
 * caller's stream by events; 0 after it; 2, the default, forks when
 * "lane_blocks" caps the encoder's grid and the caller's stream has neither a
 * CU mask nor a non-default priority, which the fork's stream would escape).
 * "acl_inplace" (1 default, 0 off): the decode calls
 * (honu_decode_parse/fill/tables/records/batch) return an ACL list whose
 * entries are all present in place (HONU_ACL_INPLACE, see honu_meta) instead
 * of copying it into the ACL table; 0 returns every list in the table.
 * "regions_inplace" (1 default, 0 off): the same calls return every
 * non-empty region list in place (HONU_REGIONS_INPLACE) instead of in the
 * region table; 0 returns every list in the table. With both in place a
 * zero-copy batch whose ACL lists hold no nil entry writes no table entry,
 * and the single-launch decode's 64-record tiles then need no offsets from
 * their predecessors (only the batch's last tile resolves them, for
 * d_totals).
 * "inline_recovery" (kept for compatibility: 0 only): a misspeculated
 * single-launch decode is always redone by the guarded second launch; redoing
 * it inside the speculative launch measured slower in the common, clean case
 * and is gone. "recoveries" (get only): the recovery launches the context has
 * run. */
int32_t honu_ctx_set_param(honu_ctx *ctx, const char *name, int64_t value);

/* The current value of a parameter of honu_ctx_set_param, and
 * "speculate_backoff": how many of the context's next decode calls run
 * without speculation (16 once a recovery launch has run, see
 * honu_decode_records; the count drops by one per call), and
 * "walk_flag_checks" (as built): which entry flags of a speculated ACL list
 * the walk checks itself, so that a nil entry there costs no recovery launch —
 * bit 0 the first ones (the window at the tail's start), bit 1 the last ones
 * (the window after the list); the flags in between are the burst's. */
int32_t honu_ctx_get_param(const honu_ctx *ctx, const char *name, int64_t *value);

/* ABI self-description, used by bindings to check struct layouts. */
uint32_t honu_abi_version(void);
uint64_t honu_sizeof_meta(void);
uint64_t honu_sizeof_acl(void);
uint64_t honu_sizeof_collection(void);
uint64_t honu_sizeof_index(void);
uint64_t honu_sizeof_record_info(void);
uint64_t honu_sizeof_seek(void);
const char *honu_status_string(int32_t status);
/* Text of the last call-level failure on this thread (HIP error text etc.). */
const char *honu_last_error(void);

/* ------------------------------------------------------------------------ */
/* Encode: object.Marshal over a batch (object.go:24-45)                     */
/* ------------------------------------------------------------------------ */

/* Exact encoded length of every record: 1 + uvarint(len data) + len data +
 * 1 + len(Metadata encoding) (object.go:30,35,40). A record that cannot be
 * encoded gets size 0 and d_status[i] = HONU_ERR_PANIC when HONU_HAS_META is
 * clear (Marshal(nil, …) dereferences nil, metadata.go:66) or HONU_ERR_INPUT
 * when a span or list lies outside its arena; otherwise d_status[i] = HONU_OK.
 * A span is validated only when its struct's presence bit is set, as Go never
 * reads a nil struct's fields; mime is always live.
 * Arguments as for honu_encode. */
int32_t honu_encode_sizes(honu_ctx *ctx, const honu_meta *d_meta, uint64_t var_len,
                          const honu_acl *d_acl, uint64_t acl_len, const uint32_t *d_regions,
                          uint64_t regions_len, const uint64_t *d_payload_off, uint64_t n,
                          uint64_t *d_sizes, int32_t *d_status, void *stream);

/* Exclusive prefix sum: d_out[i] = sum(d_in[0..i)), d_out[n] = total
 * (d_out[0] = 0 for n == 0). d_out must hold n+1 values and may alias d_in
 * only if equal. Exact in uint64 arithmetic (modulo 2^64, as a serial sum)
 * for up to 2^33 rows: the words that carry a tile's sum to the tiles after
 * it hold 43 value bits, so the sum travels as three limbs. (The decode's
 * internal three-column scans carry whole sums: table entries and data-arena
 * bytes of one batch, exact while each total stays below 2^43 = 8 TiB.)
 * n above the context's max_records returns HONU_E_WORKSPACE and stores
 * nothing. */
int32_t honu_exclusive_scan(honu_ctx *ctx, const uint64_t *d_in, uint64_t n, uint64_t *d_out,
                            void *stream);

/* Encode record i into d_out[d_out_off[i], d_out_off[i+1]). d_out_off comes
 * from honu_encode_sizes + honu_exclusive_scan and d_status from
 * honu_encode_sizes: records whose status is not HONU_OK are skipped, records
 * whose range exceeds out_cap get HONU_ERR_CAPACITY; nothing is written for a
 * failed record.
 *   d_var, var_len:        byte arena indexed by honu_meta spans
 *   d_acl, acl_len:        ACL table indexed by acl_off/acl_count
 *   d_regions, regions_len: uint32 region table
 *   d_payload, d_payload_off: CSR payload arena (the `data` argument)
 * honu_encode = honu_encode_records (header + Metadata tail of every record)
 * followed by honu_encode_payloads (the payload bytes, object.go:35); the two
 * phases are exported separately so they can be scheduled and timed apart. */
int32_t honu_encode(honu_ctx *ctx, const honu_meta *d_meta, const uint8_t *d_var, uint64_t var_len,
                    const honu_acl *d_acl, uint64_t acl_len, const uint32_t *d_regions,
                    uint64_t regions_len, const uint8_t *d_payload, const uint64_t *d_payload_off,
                    uint64_t n, uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_off,
                    int32_t *d_status, void *stream);
int32_t honu_encode_records(honu_ctx *ctx, const honu_meta *d_meta, const uint8_t *d_var,
                            const honu_acl *d_acl, const uint32_t *d_regions,
                            const uint64_t *d_payload_off, uint64_t n, uint8_t *d_out,
                            uint64_t out_cap, const uint64_t *d_out_off, int32_t *d_status,
                            void *stream);
/* honu_encode_payloads needs only d_out_off and the size pass's d_status, so it
 * may run on another stream beside honu_encode_records (each writes only its
 * own bytes of the shared 16-byte chunks); it repeats the out_cap check
 * itself and copies nothing for a record that ends past out_cap. */
int32_t honu_encode_payloads(honu_ctx *ctx, const uint8_t *d_payload, const uint64_t *d_payload_off,
                             uint64_t n, uint8_t *d_out, uint64_t out_cap,
                             const uint64_t *d_out_off, const int32_t *d_status, void *stream);
/* The same two phases split at the memory side's 64-byte write unit (ABI 5):
 * honu_encode_records_units also writes each payload's bytes in the partial
 * 64-byte units at its two ends (from d_payload), and honu_encode_payloads_units
 * writes the whole units between, so no 64-byte unit of the records arena is
 * written partly by both phases (a unit that leaves L2 partly written costs a
 * read-modify-write: DESIGN §3 "the 64-byte write unit"; 1M Small step -1.6 %).
 * Units are counted on absolute addresses of d_out. Records encoded by one of
 * the pair are completed only by the other: never mix the two forms on a
 * batch. honu_encode (one call) uses this form. */
int32_t honu_encode_records_units(honu_ctx *ctx, const honu_meta *d_meta, const uint8_t *d_var,
                                  const honu_acl *d_acl, const uint32_t *d_regions,
                                  const uint8_t *d_payload, const uint64_t *d_payload_off, uint64_t n,
                                  uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_off,
                                  int32_t *d_status, void *stream);
int32_t honu_encode_payloads_units(honu_ctx *ctx, const uint8_t *d_payload, const uint64_t *d_payload_off,
                                   uint64_t n, uint8_t *d_out, uint64_t out_cap,
                                   const uint64_t *d_out_off, const int32_t *d_status, void *stream);

/* sizes + scan + encode in one call; d_out_off (n+1) is produced here. */
int32_t honu_marshal_batch(honu_ctx *ctx, const honu_meta *d_meta, const uint8_t *d_var,
                           uint64_t var_len, const honu_acl *d_acl, uint64_t acl_len,
                           const uint32_t *d_regions, uint64_t regions_len,
                           const uint8_t *d_payload, const uint64_t *d_payload_off, uint64_t n,
                           uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off,
                           int32_t *d_status, void *stream);

/* ------------------------------------------------------------------------ */
/* Decode: Object.Metadata() + Object.Data() over a batch (object.go:66-99)  */
/* ------------------------------------------------------------------------ */

/* Phase 1: parse every record of the CSR batch (d_rec, d_rec_off[n+1]):
 * header, payload descriptor and the full Metadata walk with the exact
 * lani error semantics. Writes d_meta rows (list counts set, list offsets
 * not yet) and d_info. List positions and counts are kept in the context. */
int32_t honu_decode_parse(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                          uint64_t n, honu_meta *d_meta, honu_record_info *d_info, void *stream);

/* Phase 2: assign table offsets (exclusive scans over the counts), fill
 * the ACL and region tables, and when d_data != NULL assign every payload a
 * 16-byte aligned offset in d_data (d_info[i].data_off is then relative to
 * d_data) and copy the payloads there (honu_decode_payloads). d_totals
 * (device, 3 x u64) receives the totals the batch needs: ACL table entries
 * (lists returned in place take none), region table entries (likewise),
 * data-arena bytes (the latter also in zero-copy mode). Rows returned with
 * in-place lists (and every span) point into d_rec: keep the records arena
 * alive while the rows are used. Records whose
 * outputs do not fit get HONU_ERR_CAPACITY in meta_status / data_status. */
int32_t honu_decode_fill(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                         uint64_t n, honu_meta *d_meta, honu_record_info *d_info,
                         honu_acl *d_acl, uint64_t acl_cap, uint32_t *d_regions,
                         uint64_t regions_cap, uint8_t *d_data, uint64_t data_cap,
                         uint64_t *d_totals, void *stream);
/* honu_decode_fill without the payload copy, and the copy alone (after
 * honu_decode_tables with the same d_data and d_totals). */
int32_t honu_decode_tables(honu_ctx *ctx, const uint8_t *d_rec, uint64_t n, honu_meta *d_meta,
                           honu_record_info *d_info, honu_acl *d_acl, uint64_t acl_cap,
                           uint32_t *d_regions, uint64_t regions_cap, uint8_t *d_data,
                           uint64_t data_cap, uint64_t *d_totals, void *stream);
int32_t honu_decode_payloads(honu_ctx *ctx, const uint8_t *d_rec, uint64_t n,
                             const honu_record_info *d_info, uint8_t *d_data,
                             const uint64_t *d_totals, void *stream);

/* Parse + tables in ONE launch (the default batch decode): every output of
 * honu_decode_parse + honu_decode_tables — rows with their list offsets,
 * record info, ACL and region tables, d_totals — from a single pass over each
 * record's header and Metadata tail. With materialize != 0 every payload also
 * gets its 16-byte aligned data-arena offset (d_info[i].data_off, checked
 * against data_cap) and honu_decode_payloads (same context, same d_totals)
 * then copies the payloads; with materialize == 0 Data() stays the zero-copy
 * subslice of the records arena (Object.Data, object.go:85-99). Results are
 * identical to the split path's. Launches of 768 or more 64-record tiles
 * speculate (counts published before the walk ends, ACL entry flags checked
 * by the table fill or a gather after the publish) when the param
 * "speculate" allows it — by default materialising calls and the table forms,
 * not a zero-copy call with both lists in place; a batch holding any record that fails after its counts
 * were published, or a nil ACL entry past the list's first bytes (those the
 * walk has at hand are checked at once), is decoded a second time without
 * speculation inside the same call, so such a batch costs about twice a
 * clean one (malformed input and nil entries only; results are exact either
 * way). A recovery that ran sets a pinned word of the context, and the
 * context's next 16 calls after the host sees it do not speculate (no
 * recovery launch: about 1.1x a speculative clean call), so a stream of such
 * batches does not pay twice per batch. */
int32_t honu_decode_records(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                            uint64_t n, honu_meta *d_meta, honu_record_info *d_info,
                            honu_acl *d_acl, uint64_t acl_cap, uint32_t *d_regions,
                            uint64_t regions_cap, int32_t materialize, uint64_t data_cap,
                            uint64_t *d_totals, void *stream);

/* parse + fill in one call: from 48 K records honu_decode_records (+
 * honu_decode_payloads when d_data != NULL), below the split phases. */
int32_t honu_decode_batch(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                          uint64_t n, honu_meta *d_meta, honu_record_info *d_info,
                          honu_acl *d_acl, uint64_t acl_cap, uint32_t *d_regions,
                          uint64_t regions_cap, uint8_t *d_data, uint64_t data_cap,
                          uint64_t *d_totals, void *stream);

/* Object.StorageVersion() / Data() / Tombstone() (object.go:47-52,85-112)
 * without Metadata(): every honu_record_info field but meta_status, which is
 * HONU_UNPARSED. Reads only each record's header (version byte + the
 * dataLength varint): the Collection.Exists path (collection.go:55-65). */
int32_t honu_decode_headers(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                            uint64_t n, honu_record_info *d_info, void *stream);

/* Object.Data() (object.go:85-99) of every record materialised into a packed
 * data arena, without Metadata(): Data() needs only the header, so this runs
 * beside (on another stream and context) or without a Metadata() parse. d_info
 * is written as by honu_decode_headers, except that data_off is relative to
 * d_data: payloads are 16-byte aligned and back to back in record order, the
 * offsets honu_decode_fill assigns. A payload that does not fit data_cap gets
 * HONU_ERR_CAPACITY in data_status and is not copied. d_totals (optional,
 * device, 1 x u64) receives the data-arena bytes the batch needs. */
int32_t honu_decode_data(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                         uint64_t n, honu_record_info *d_info, uint8_t *d_data, uint64_t data_cap,
                         uint64_t *d_totals, void *stream);
/* honu_decode_data in two phases, to schedule or time the copy apart: place
 * (header walk, offsets, capacity; d_info complete after it) and the payload
 * copy (same ctx and d_info, after place on the same stream). */
int32_t honu_decode_data_place(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                               uint64_t n, honu_record_info *d_info, uint64_t data_cap,
                               uint64_t *d_totals, void *stream);
int32_t honu_decode_data_copy(honu_ctx *ctx, const uint8_t *d_rec, uint64_t n,
                              const honu_record_info *d_info, uint8_t *d_data, void *stream);

/* Object.Key() (object.go:57-64 -> keys.New, keys/keys.go:42-51) for every
 * decoded record: 0x01 | ObjectID | BE64(VID) | BE32(PID), 29 bytes per
 * record at d_keys + 29*i. d_key_status[i] = meta_status, or HONU_ERR_PANIC
 * when the decoded Version is nil (metadata.go:54 dereferences it). */
int32_t honu_decode_keys(honu_ctx *ctx, const honu_meta *d_meta, const honu_record_info *d_info,
                         uint64_t n, uint8_t *d_keys, int32_t *d_key_status, void *stream);

/* Bytes of caller-owned device workspace that honu_sort_keys and
 * honu_key_objects need for n keys (one workspace serves both): a multiple of
 * 256, monotonic in n, at most 96 n + 2^20. The workspace itself must be
 * 256-byte aligned (hipMalloc gives that). The context's own allocations do
 * not grow with these calls. Needs no device. */
uint64_t honu_sort_keys_workspace(uint64_t n);

/* sort.Sort(keys.Keys) (keys/keys.go:126-130: Less is bytes.Compare < 0),
 * made deterministic: a stable sort of the key column honu_decode_keys writes
 * (29 bytes per key at d_keys + 29*i, any byte alignment) over all 29 bytes.
 * Key i takes part when d_key_status is NULL or d_key_status[i] == HONU_OK.
 * d_order[0, valid) receives the indices of the valid keys in ascending key
 * order, equal keys in ascending index; d_order[valid, n) the other indices,
 * ascending: always a permutation of 0..n-1. d_sorted (optional, 29 n bytes):
 * row p is d_keys row d_order[p], for every p < n. d_valid[0] = valid. With
 * n == 0 only d_valid[0] = 0 is written. Asynchronous on `stream`, no host
 * synchronisation, replays from a captured graph; uses the context's scan
 * state (one context per concurrent stream). Refusals, each storing nothing:
 * HONU_E_WORKSPACE for n above honu_ctx_max_records or above 2^32 - 1;
 * HONU_E_ARG for work_bytes below honu_sort_keys_workspace(n), a NULL or
 * misaligned workspace, or NULL d_keys, d_order (n > 0) or d_valid.
 * The get-only param "sort_tile" is the keys one workgroup takes per pass. */
int32_t honu_sort_keys(honu_ctx *ctx, const uint8_t *d_keys, const int32_t *d_key_status,
                       uint64_t n, uint32_t *d_order, uint8_t *d_sorted, uint64_t *d_valid,
                       void *d_work, uint64_t work_bytes, void *stream);

/* The objects of a sorted key column with their versions: what a read of
 * "the latest version ... or all versions related to the object"
 * (keys.go:40-41) ranges over, [ObjectPrefix, ObjectLimit) (keys.go:73-92).
 * The positions p < d_valid[0] of d_order (both as honu_sort_keys wrote them;
 * d_valid is read on the device, so the call follows the sort on the same
 * stream with no host round trip) are cut where key[0:17] changes.
 * d_obj_off (room for n + 1 values; objects + 1 are written): the versions of
 * object j are d_order[d_obj_off[j], d_obj_off[j+1]), oldest first by
 * lamport.Compare (lamport/scalar.go:50-78: VID, then PID), and
 * d_obj_off[objects] = valid. d_latest (optional, room for n; `objects` are
 * written): d_latest[j] = d_order[d_obj_off[j+1] - 1]. d_objects[0] =
 * objects. Groups are by equality of the 17-byte prefix: ObjectLimit()'s
 * limit[16]++ (keys.go:88-91) wraps for an object ID that ends in 0xff, which
 * leaves the reference's own range empty there; that is not reproduced.
 * Workspace, refusals and stream rules as honu_sort_keys (d_valid, d_obj_off
 * and d_objects are required; d_keys and d_order when n > 0). */
int32_t honu_key_objects(honu_ctx *ctx, const uint8_t *d_keys, const uint32_t *d_order,
                         const uint64_t *d_valid, uint64_t n, uint64_t *d_obj_off,
                         uint32_t *d_latest, uint64_t *d_objects,
                         void *d_work, uint64_t work_bytes, void *stream);

/* One row of honu_key_seek per probe. */
#define HONU_SEEK_NONE 0xFFFFFFFFu
enum {
    HONU_SEEK_FOUND       = 1u << 0, /* key != nil && bytes.HasPrefix(key, probe): Collection.Has, collection.go:49-50 */
    HONU_SEEK_END         = 1u << 1, /* Seek returned nil: pos == valid (cursor_test.go:116-121) */
    HONU_SEEK_EXACT       = 1u << 2, /* FOUND and probe_len == 29: the key itself is stored */
    HONU_SEEK_FIRST_LIVE  = 1u << 3, /* FOUND and !info[first].tombstone: Collection.Exists AS WRITTEN (collection.go:57-64
                                        reads the value at the Seek position, the object's LOWEST version) */
    HONU_SEEK_LATEST_LIVE = 1u << 4, /* FOUND and !info[latest].tombstone: Exists / Retrieve AS DOCUMENTED
                                        (collection.go:53-54, 97-101: the latest version) */
    HONU_SEEK_SKIPPED     = 1u << 5  /* d_probe_status[q] != HONU_OK: not looked up */
};
typedef struct honu_seek {
    uint32_t pos;    /* Cursor.Seek: first p in [0, valid) with bytes.Compare(sorted[p], probe) >= 0; valid when none */
    uint32_t end;    /* first p >= pos whose key does not have the probe as prefix; [pos, end) are the probe's keys */
    uint32_t first;  /* d_order[pos]     (record index), HONU_SEEK_NONE unless FOUND and d_order given */
    uint32_t latest; /* d_order[end - 1] (record index), likewise */
    uint32_t flags;
} honu_seek;         /* 20 */

/* Cursor.Seek (iterator/cursor.go:44-55; cursor_test.go:95-121: an existing
 * key, a key between two keys, a key beyond the end) for a batch of m probes
 * over a sorted key column: the step Collection.Has (collection.go:47-51),
 * Collection.Exists (collection.go:55-65) and the lookups in the collections
 * bucket (tx.go:123-125, store.go:287-288, 363-379) start from, and both ends
 * of the range [ObjectPrefix, ObjectLimit) (keys/keys.go:73-92) that
 * Retrieve and Versions (collection.go:97-110: "latest version of the
 * object", "all versions, most recent first") range over.
 * Inputs. d_sorted is the sorted column honu_sort_keys writes: 29 bytes per
 * row, any byte alignment. Only rows [0, valid) are searched, valid =
 * min(d_valid[0], n): the rows from valid on hold the bytes of invalid keys
 * and are never returned, even where they equal a probe. d_valid is read on
 * the device, so the call follows the sort on the same stream with no host
 * round trip. Probe q is the first probe_len bytes (0..29, one length per
 * call) of the 29-byte row at d_probes + 29*q, any byte alignment; all 29 m
 * bytes must be readable, so a key column of honu_decode_keys is a probe
 * column as it stands. probe_len 29 looks up a key, 17 an ObjectPrefix
 * (keys.go:74-79), 16 a bare id as Has literally passes it; 0 matches every
 * key.
 * Results. The comparison is bytes.Compare: a key that has the probe as a
 * proper prefix is greater than the probe. pos is therefore the lower bound
 * over the probe_len-byte prefixes of the keys and end the upper bound; FOUND
 * means pos < end. end stands for the second seek to ObjectLimit(), whose
 * limit[16]++ wraps for an id that ends in 0xff (keys.go:88-91); the wrap is
 * not reproduced, as in honu_key_objects. Equal keys form one run: pos its
 * first position, end the position past its last.
 * Optional inputs. d_probe_status (NULL: every probe takes part): a probe
 * whose status is not HONU_OK gets {0, 0, NONE, NONE, SKIPPED}. d_order (the
 * sort's) enables first and latest, which are its values at pos and end - 1.
 * d_info (n rows; needs d_order) enables the two LIVE bits; an index of
 * d_order that is not below n reads row n - 1 there, as in honu_key_objects.
 * d_info is indexed by record and clamped by n, the column's rows: the LIVE
 * bits answer for the column only while every index in its valid rows is below
 * n. Over a view of a bucketed column (honu_key_merge_buckets, "d_info over a
 * view") the caller has to keep that.
 * With valid == 0 every probe that takes part gets pos = end = 0 and END.
 * With m == 0 nothing is launched or stored.
 * The write set is exactly d_out[0, m). No workspace and no context scratch:
 * calls on different streams may share a context. Asynchronous on `stream`,
 * no host synchronisation, no allocation; replays from a captured graph.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for n or m above 2^32 - 1;
 * HONU_E_ARG for a NULL ctx or d_valid, a NULL d_out or d_probes with m > 0,
 * a NULL d_sorted with n > 0, probe_len > 29, d_info without d_order, or a
 * misaligned pointer (4 bytes: d_out, d_order, d_probe_status; 8 bytes:
 * d_valid, d_info).
 * Param "seek_variant": 0 auto (the default), 1 the direct binary search over
 * the column, 2 the fenced search, which resolves the top levels from "seek_fence"
 * (get only) keys that each workgroup samples into LDS; auto takes the direct
 * form for fewer than "seek_auto_probes" probes (1024) over more than
 * "seek_auto_keys" rows (65536; both get only; n stands for the valid count,
 * which the host does not know), and the fenced form otherwise. */
int32_t honu_key_seek(honu_ctx *ctx, const uint8_t *d_sorted, const uint64_t *d_valid, uint64_t n,
                      const uint8_t *d_probes, const int32_t *d_probe_status, uint32_t probe_len,
                      uint64_t m, const uint32_t *d_order, const honu_record_info *d_info,
                      honu_seek *d_out, void *stream);

/* A batch of Puts into the sorted key column: what collections.Put(key, data)
 * (store.go:232, 395), collectionsBucket.Put(collectionKey, data)
 * (store.go:530) and the 128 bkt.Put(k, value) calls of
 * iterator/cursor_test.go:235 do to an ordered bucket one key at a time, after
 * which the next Seek sees the key. The stable merge of two sorted columns.
 * Inputs. A and B are each what honu_sort_keys writes: a sorted column of
 * 29-byte rows at any byte alignment with the valid keys in [0, v), v =
 * min(d_valid[0], n), the rows of the invalid keys behind them in index
 * order, and the matching d_order. d_valid_a and d_valid_b are read on the
 * device, so the call follows the two sorts, or an earlier merge, on the same
 * stream with no host round trip. b_base is added to every index taken from
 * d_order_b: the number of records that precede B's in the caller's
 * concatenated record arrays, na for a first merge of two sorts, the running
 * total when chaining.
 * Outputs, rows and indices [0, na + nb), and d_valid_out[0] = va + vb.
 * Positions [0, va + vb) hold the stable merge of A's valid rows and B's by
 * bytes.Compare: on equal keys every A row precedes every B row, and each
 * side keeps its own order. The tail [va + vb, na + nb) is A's invalid rows
 * [va, na), then B's [vb, nb), their bytes as they stand, their indices
 * unchanged for A and + b_base for B. With b_base = na every output equals,
 * bit for bit, what honu_sort_keys returns for the concatenated key and
 * status columns (that sort is stable and puts equal keys in ascending
 * index), so the result is fit for honu_key_seek, honu_key_objects and a
 * further honu_key_merge.
 * Put semantics. bbolt's Put of a stored key replaces its value. Here equal
 * keys stay one run, as they do after honu_sort_keys, and the run's last row
 * is the latest arrival: what honu_seek.latest, d_order[end - 1], returns.
 * d_order_out may be NULL: d_order_a and d_order_b are then ignored and only
 * the column is merged. Given, it needs both input orders.
 * The write set is exactly d_sorted_out[0, 29 (na + nb)), d_order_out[0, na +
 * nb) and d_valid_out[0]; the outputs must not overlap the inputs. With na +
 * nb == 0 only d_valid_out[0] = 0 is written. No workspace and no context
 * scratch: calls on different streams may share a context. Asynchronous on
 * `stream`, no host synchronisation, no allocation; replays from a captured
 * graph.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for na + nb above 2^32 - 1;
 * HONU_E_ARG for a NULL ctx, d_valid_a, d_valid_b or d_valid_out, a NULL
 * column or output column with a non-zero count, d_order_out without both
 * input orders, b_base + nb above 2^32 - 1, or a misaligned pointer (4 bytes:
 * the orders; 8 bytes: the valid counts).
 * The get-only param "merge_tile" is the output positions one workgroup
 * produces. */
int32_t honu_key_merge(honu_ctx *ctx, const uint8_t *d_sorted_a, const uint32_t *d_order_a,
                       const uint64_t *d_valid_a, uint64_t na, const uint8_t *d_sorted_b,
                       const uint32_t *d_order_b, const uint64_t *d_valid_b, uint64_t nb,
                       uint32_t b_base, uint8_t *d_sorted_out, uint32_t *d_order_out,
                       uint64_t *d_valid_out, void *stream);

/* honu_key_delete flags */
enum { HONU_DELETE_SUPERSEDED = 1u << 0 /* also remove every row that the next valid row repeats */ };

/* Bytes of honu_key_delete's workspace for a column of n rows: a multiple of
 * 256, monotonic in n, 0 for n == 0; needs no device. */
uint64_t honu_key_delete_workspace(uint64_t n);

/* A batch of Deletes from the sorted key column: what the loop "Delete all
 * collection versions" of Store.Drop (store.go:378-383: cursor.Seek(id[:]),
 * then collections.Delete(key) while bytes.HasPrefix(key, id[:])) and the
 * tx.DeleteBucket behind it (store.go:399-404) do to an ordered bucket one key
 * at a time, and what every Put of a stored key does to the row it replaces.
 * A stable compaction of the column.
 * Inputs. The column is what honu_sort_keys or honu_key_merge writes: n rows
 * of 29 bytes at any byte alignment, the valid keys in [0, v), v =
 * min(d_valid[0], n), and the matching d_order. The delete list is a sorted
 * column of the same kind, a honu_sort_keys output over the keys to delete: m
 * rows, of which [0, vd) count, vd = min(d_valid_del[0], m). Both counts are
 * read on the device, so the call follows the sorts, a merge or an earlier
 * delete on the same stream with no host round trip. Only the first probe_len
 * bytes (0..29, one length per call) of a delete row count, as in
 * honu_key_seek: 29 is bucket.Delete(key), 17 an ObjectPrefix (keys.go:74-79),
 * 16 the bare id as store.go:379 literally passes it, and 0 with vd >= 1
 * removes every valid row (the DeleteBucket of store.go:402, a Truncate). A
 * column sorted over 29 bytes is sorted over every prefix length, so the list
 * needs no second sort. Delete rows may repeat; one that matches nothing is
 * not an error, as bbolt's Delete of an absent key returns nil. m == 0 with
 * d_del and d_valid_del NULL is allowed.
 * Which rows go. A valid row p < v is removed when (a) its first probe_len
 * bytes equal those of some delete row in [0, vd), or (b)
 * HONU_DELETE_SUPERSEDED is set, p + 1 < v and row p + 1 has the same 29
 * bytes: a later arrival replaced it (the Put semantics of honu_key_merge), so
 * of a run of equal keys only the last row stays, the one honu_seek.latest
 * names. Rows of the column at or past v and delete rows at or past vd take
 * no part, even where their bytes match.
 * Outputs, n rows and n indices, always a permutation of the input's: [0,
 * kept) the rows that stay, in column order; [kept, kept + removed) the rows
 * that go, in column order, whose d_order_out values are the record indices
 * whose values a caller frees; [v, n) the invalid tail as it stands.
 * d_valid_out[0] = kept and, where d_removed is given, d_removed[0] = removed
 * = v - kept, so the result is fit for honu_key_seek, honu_key_objects,
 * honu_key_merge and a further honu_key_delete. d_order_out may be NULL:
 * d_order is then ignored and only the column is compacted. Given, it needs
 * d_order.
 * As written and as documented. The loop at store.go:379-383 calls
 * bucket.Delete while it walks with cursor.Next(), which bbolt documents as
 * able to skip keys. This call does what the loop states ("Delete all
 * collection versions"): every key with the prefix goes.
 * The write set is exactly d_sorted_out[0, 29 n), d_order_out[0, n),
 * d_valid_out[0] and d_removed[0], besides the workspace; the outputs must not
 * overlap the inputs. With n == 0 only the two counts (0) are written.
 * d_work is honu_key_delete_workspace(n) bytes, 256-byte aligned (unused,
 * and NULL allowed, when that is 0). The kept counts of the tiles, one per
 * "delete_tile" rows, are summed by the context's scan (the one behind
 * honu_exclusive_scan), whose state covers max_records rows: the column may
 * have up to "delete_tile" * max_records rows (1024 rows per record the
 * context was created for), and one context serves one stream at a time, as
 * for honu_sort_keys. Asynchronous on
 * `stream`, no host synchronisation, no allocation; replays from a captured
 * graph, with the counts changed on the device between replays.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for n or m above 2^32 - 1,
 * or for n above "delete_tile" * max_records (more tiles than the context's
 * scan covers; honu_sort_keys refuses n above max_records the same way);
 * HONU_E_ARG for a NULL ctx, d_valid or d_valid_out, a NULL d_valid_del or
 * d_del with m > 0, a NULL column or output column with n > 0, d_order_out
 * without d_order with n > 0, probe_len > 29, unknown flag bits, work_bytes
 * below honu_key_delete_workspace(n), a NULL or misaligned (256) workspace
 * when that size is not 0, or a misaligned pointer (4 bytes: the orders; 8
 * bytes: the counts).
 * The get-only param "delete_tile" is the column positions one workgroup
 * takes. */
int32_t honu_key_delete(honu_ctx *ctx, const uint8_t *d_sorted, const uint32_t *d_order,
                        const uint64_t *d_valid, uint64_t n, const uint8_t *d_del,
                        const uint64_t *d_valid_del, uint64_t m, uint32_t probe_len, uint32_t flags,
                        uint8_t *d_sorted_out, uint32_t *d_order_out, uint64_t *d_valid_out,
                        uint64_t *d_removed, void *d_work, uint64_t work_bytes, void *stream);

/* honu_key_list flags */
enum {
    HONU_LIST_REVERSE = 1u << 0, /* Prev() from the range's last row: end-1 down to pos (Versions: most recent first) */
    HONU_LIST_LATEST  = 1u << 1  /* one row per object: only rows that are the last of their 17-byte prefix group */
};
enum {                            /* honu_list_row.flags */
    HONU_LIST_ROW_HEAD      = 1u << 0, /* first row emitted for its range */
    HONU_LIST_ROW_TOMBSTONE = 1u << 1  /* d_info given and info[record].tombstone */
};
typedef struct honu_list_row {
    uint32_t range;   /* q: which honu_seek row it came from */
    uint32_t pos;     /* position in the sorted column */
    uint32_t record;  /* d_order[pos]; HONU_SEEK_NONE when d_order is NULL */
    uint32_t flags;
} honu_list_row;      /* 16 */
uint64_t honu_sizeof_list_row(void);

/* A batch of cursor walks over the sorted key column: every reference read
 * path after the Seek is a walk with Cursor.Next() or Cursor.Prev()
 * (iterator/cursor.go:57-89): Collection.List() (collection.go:32-35),
 * Versions() ("from the most recent version to the oldest",
 * collection.go:106-110), Retrieve() ("the latest version",
 * collection.go:97-104) and the loop `for ; key != nil &&
 * bytes.HasPrefix(key, id[:]); key, _ = cursor.Next()` of store.go:379. For m
 * ranges, given as the honu_seek rows honu_key_seek wrote, the call emits
 * every row that a cursor walking each range would visit, packed, the ranges
 * in order. Every count stays on the device.
 * Range bounds. v = min(d_valid[0], n). Range q uses end' = min(end, v) and
 * pos' = min(pos, end') of d_ranges[q]; a range whose flags carry
 * HONU_SEEK_SKIPPED is empty. No other flag bit of the seek row is trusted
 * and neither are first and latest: only pos and end are read. Ranges may
 * overlap, repeat and come in any order.
 * Plain mode. c_q = end' - pos', capped at limit when limit != 0 (limit
 * stands for calling Next() that many times). The positions are pos', pos' +
 * 1, ...; with HONU_LIST_REVERSE end' - 1, end' - 2, ... (Prev()), so limit 1
 * with REVERSE is Retrieve's latest version of an object range.
 * HONU_LIST_LATEST. Needs d_obj_off and d_objects as honu_key_objects wrote
 * them for this column (objects + 1 offsets, d_obj_off[objects] = valid; room
 * for n + 1 values). It reads objects = min(d_objects[0], n) and clamps every
 * offset to v. The candidate rows are L_j = d_obj_off[j + 1] - 1, each
 * object's last row; range q emits the L_j with pos' <= L_j < end', ascending
 * j, descending with REVERSE, and limit applies after that. An object whose
 * latest version lies outside the range is not emitted.
 * Tombstones. Collection.Delete's comment says an object with a tombstone
 * version "will not be returned in list queries" (collection.go:132-134).
 * Here a tombstone is FLAGGED (HONU_LIST_ROW_TOMBSTONE, when d_info is
 * given), not filtered: honu_key_filter compacts the flagged rows, or every
 * row of a deleted object, out of the list (honu_key_fetch with
 * HONU_FETCH_LIVE fetches nothing for a flagged row and leaves the row in
 * place).
 * Outputs. d_range_off[0, m] is the exclusive scan of the c_q and
 * d_range_off[m] = d_total[0] = total, a 64-bit sum (overlapping ranges can
 * exceed n). w = min(total, cap): only output rows g < w are written. Row g
 * belongs to the range q with d_range_off[q] <= g < d_range_off[q + 1] and
 * its position is the (g - d_range_off[q])-th of that range; HEAD is set on
 * the 0-th. d_rows[g] is written whole; d_keys_out + 29 g, when given,
 * receives the 29 bytes of the column's row (Cursor.Key()'s copy). A caller
 * that sees total > cap re-issues with more room. The write set is exactly
 * d_range_off[0, m + 1), d_total[0], d_rows[0, w) and d_keys_out[0, 29 w).
 * Optionals. d_order, d_info and d_keys_out may be NULL; d_info needs
 * d_order. Without d_order, record is HONU_SEEK_NONE. An index of d_order
 * that is not below n reads d_info row n - 1, as in honu_key_seek: d_info is
 * indexed by record and clamped by the column's rows, so TOMBSTONE answers for
 * the column only while every index in its valid rows is below n (over a view
 * of a bucketed column see honu_key_merge_buckets, "d_info over a view"). d_rows may
 * be NULL only with cap == 0: a counting call. With m == 0, d_range_off[0] =
 * 0 and d_total[0] = 0; with v == 0 every count is 0.
 * Asynchronous on `stream`, no host synchronisation, no allocation, no
 * workspace; replays from a captured graph, also after the counts and seek
 * rows were changed on the device between replays. The counts are scanned in
 * place in d_range_off by the context's scan (the one behind
 * honu_exclusive_scan), so one context serves one stream at a time, as for
 * honu_sort_keys and honu_key_delete. Garbage in d_ranges or d_obj_off may
 * give wrong rows, never an access outside the n rows or a search that does
 * not end.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for n, m or cap above
 * 2^32 - 1, or for m + 1 above honu_ctx_max_records; HONU_E_ARG for a NULL
 * ctx, d_valid, d_range_off or d_total, a NULL d_ranges with m > 0, a NULL
 * d_sorted with n > 0, a NULL d_rows with cap > 0, unknown flag bits, LATEST
 * without both d_obj_off and d_objects, d_info without d_order, or a
 * misaligned pointer (4 bytes: d_ranges, d_order; 8 bytes: d_valid,
 * d_objects, d_obj_off, d_range_off, d_total, d_info; 16 bytes: d_rows).
 * The get-only params are "list_tile" (output rows per workgroup) and
 * "list_stage" (range offsets a workgroup stages in LDS). */
int32_t honu_key_list(honu_ctx *ctx, const uint8_t *d_sorted, const uint32_t *d_order,
                      const uint64_t *d_valid, uint64_t n,
                      const honu_seek *d_ranges, uint64_t m, uint32_t limit, uint32_t flags,
                      const uint64_t *d_obj_off, const uint64_t *d_objects,   /* LATEST only */
                      const honu_record_info *d_info,
                      uint64_t *d_range_off, honu_list_row *d_rows, uint8_t *d_keys_out,
                      uint64_t cap, uint64_t *d_total, void *stream);

/* honu_key_fetch flags */
enum {
    HONU_FETCH_LIVE = 1u << 0 /* rows flagged HONU_LIST_ROW_TOMBSTONE fetch nothing */
};

/* Cursor.Object() over listed rows: the step every reference read path ends
 * in. Object() (iterator/cursor.go:31-38) is make + copy of the value under
 * the cursor, once per row that List, Versions or Retrieve visits
 * (collection.go:32-35, 97-110). For the rows honu_key_list wrote, the call
 * copies the record each row names out of a CSR records arena into a packed
 * CSR arena of its own (d_values, d_val_off): the input form of
 * honu_decode_batch, honu_decode_headers and honu_decode_data, so seek, list,
 * fetch and decode run on one stream with nothing read on the host. Every
 * count stays on the device.
 * Inputs. d_rows, d_total and cap are what honu_key_list wrote and was given:
 * w = min(d_total[0], cap) is read on the device and only rows g < w take
 * part. d_rec, d_rec_off[nrec + 1] are the records arena (any byte
 * alignment), rec_bytes its readable size.
 * Lengths. Row g < w names r = d_rows[g].record. With HONU_FETCH_LIVE and
 * HONU_LIST_ROW_TOMBSTONE in d_rows[g].flags its length is 0 and its status
 * HONU_OK, whatever r is, and d_rec_off is not read: Object() returning nil
 * for the object that a listing does not return (collection.go:132-134). The
 * row stays in place; honu_key_filter before the fetch takes it out of the
 * list. Otherwise r >= nrec
 * (HONU_SEEK_NONE of a list made without d_order included) gives length 0 and
 * HONU_ERR_INPUT; otherwise a = d_rec_off[r], b = d_rec_off[r + 1] give length
 * b - a and HONU_OK when a <= b <= rec_bytes, else length 0 and
 * HONU_ERR_INPUT. Rows g >= w have length 0 and no status. Rows may repeat a
 * record (overlapping ranges do): its bytes are then read twice.
 * Outputs. d_val_off[0, cap] is the exclusive scan of the lengths, packed with
 * no padding, and d_val_off[cap] = d_val_total[0] the bytes the rows need.
 * Row g is copied to d_values + d_val_off[g] exactly when its length is not 0
 * and d_val_off[g + 1] <= val_cap; the offsets are monotone, so the copied
 * rows are a prefix. A caller that reads d_val_total[0] > val_cap re-issues
 * with more room, as with the list's cap: a prefix rule, not a status per row.
 * The write set is exactly d_val_off[0, cap + 1), d_val_total[0],
 * d_status[0, w) (d_status may be NULL) and the bytes of the copied rows in
 * d_values. With cap == 0 only d_val_off[0] = 0 and d_val_total[0] = 0 are
 * written. d_values may be NULL only with val_cap == 0: a sizing call.
 * Asynchronous on `stream`, no host synchronisation, no allocation, no
 * workspace beyond the outputs; replays from a captured graph, also after
 * d_total and the rows were changed on the device between replays. The
 * lengths are scanned in place in d_val_off by the context's scan, so one
 * context serves one stream at a time, as for honu_key_list; the copy takes a
 * line of the context's copy counters like every payload copy. Garbage in
 * d_rows or d_rec_off may give wrong bytes, never a read of d_rec_off outside
 * [0, nrec], a read of a record byte outside [0, rec_bytes) or a write outside
 * the write set (the copy loads whole aligned 16-byte blocks that hold at
 * least one byte of a record it copies, as every payload copy does).
 * Refusals, each storing nothing: HONU_E_WORKSPACE for cap or nrec above
 * 2^32 - 1, or for cap + 1 above honu_ctx_max_records; HONU_E_ARG for a NULL
 * ctx, d_total, d_val_off or d_val_total, a NULL d_rows with cap > 0, a NULL
 * d_rec_off, a NULL d_rec with rec_bytes > 0, a NULL d_values with val_cap >
 * 0, unknown flag bits, or a misaligned pointer (4 bytes: d_status; 8 bytes:
 * d_total, d_rec_off, d_val_off, d_val_total; 16 bytes: d_rows). */
int32_t honu_key_fetch(honu_ctx *ctx, const honu_list_row *d_rows, const uint64_t *d_total,
                       uint64_t cap,
                       const uint8_t *d_rec, const uint64_t *d_rec_off, uint64_t nrec,
                       uint64_t rec_bytes, uint32_t flags,
                       uint64_t *d_val_off, int32_t *d_status,
                       uint8_t *d_values, uint64_t val_cap, uint64_t *d_val_total, void *stream);

/* honu_key_filter flags */
enum {
    HONU_FILTER_TOMBSTONE = 1u << 0, /* drop a row whose flags carry HONU_LIST_ROW_TOMBSTONE */
    HONU_FILTER_DELETED   = 1u << 1  /* drop every row of an object whose LATEST version is a tombstone */
};

/* Bytes of honu_key_filter's workspace for a list of cap rows: a multiple of
 * 256, monotonic in cap, 0 for cap == 0; needs no device. */
uint64_t honu_key_filter_workspace(uint64_t cap);

/* The live-object filter over listed rows. Collection.Delete's comment says
 * that an object deleted with a tombstone version "will not be returned in
 * list queries or retrieval" (collection.go:132-134), and Retrieve of it is
 * "not found" (collection.go:97-101, 53-54). honu_key_list only flags such
 * rows; this call takes them out: a stable compaction of the list's rows, with
 * the ranges' offsets and the HEAD flags recomputed. Its output is a list
 * again (d_rows_out, d_range_off_out, d_total_out and, optionally, the keys),
 * so honu_key_fetch and the decoders take it unchanged: a range that comes out
 * empty is Retrieve's "not found", and the decoded batch holds exactly the
 * objects a reference listing returns. Every count stays on the device.
 * Rows that take part. d_rows, d_range_off[0, m], d_total and cap are what
 * honu_key_list wrote and was given; d_keys, when given, its d_keys_out. w =
 * min(d_total[0], cap) is read on the device and only rows g < w take part: a
 * truncated list is filtered as far as it was written.
 * Which rows go. Row g goes when any flag that is set says so; with flags == 0
 * the call copies the list.
 * HONU_FILTER_TOMBSTONE: the row goes when d_rows[g].flags carries
 * HONU_LIST_ROW_TOMBSTONE (the list was made with d_info). Nothing else is
 * read. This is the row's own record: right for a list whose rows are latest
 * versions (HONU_LIST_LATEST, or REVERSE with limit 1 over object ranges).
 * HONU_FILTER_DELETED: the object-level answer, for Versions of a deleted
 * object and for a List() over the whole column without LATEST, where a
 * range need not end on the object's latest version. It reads the column's
 * d_valid and n and what honu_key_objects wrote for it (d_obj_off, d_latest,
 * d_objects), and the d_info the list's records index: v = min(d_valid[0], n)
 * and objects = min(d_objects[0], n). A row with pos >= v names no object and
 * stays, and so does every row when objects == 0. Otherwise j is the object
 * with d_obj_off[j] <= pos < d_obj_off[j + 1], found by an upper bound of pos
 * over d_obj_off[1..objects], every offset clamped to v, as the list's LATEST
 * mode reads them (a pos at or past the last offset reads the last object). r
 * = d_latest[j]; an r that is not below n reads info row n - 1, the convention
 * of honu_key_seek and honu_key_list, and with the same condition: d_info is
 * indexed by record and clamped by the column's rows, so HONU_FILTER_DELETED
 * answers for the column only while every index in its valid rows is below n
 * (over a view of a bucketed column see honu_key_merge_buckets, "d_info over a
 * view"). The row goes when d_info[r].tombstone !=
 * 0. So every version row of a deleted object goes, its live older versions
 * included; a tombstone version of an object whose latest version is live
 * stays (Versions() "includes tombstone versions", collection.go:106-107);
 * and a row of an object whose latest row lies outside the row's range is
 * still judged by the column's latest row.
 * Outputs. The kept rows go to d_rows_out[0, kept) in input order. range, pos,
 * record and the TOMBSTONE bit are unchanged; every other flag bit but HEAD is
 * copied too. d_range_off_out[q], for q in [0, m), is the number of kept rows
 * among the rows below min(d_range_off[q], w), so over a list's offsets it is
 * the exclusive scan of the kept counts per range; d_range_off_out[m] =
 * d_total_out[0] = kept, whatever d_range_off[m] holds. HONU_LIST_ROW_HEAD is
 * recomputed: set on the kept row that lands on d_range_off_out[min(range, m -
 * 1)] of its own range field and cleared on every other (with m == 0 on all),
 * which over a list is exactly the first kept row of each range: HEAD moves
 * to the next kept row when a range's first row goes, and a range that
 * vanishes has none. When both key pointers are given, d_keys_out + 29 k
 * receives the 29 key bytes of the k-th kept row (any byte alignment).
 * The write set is exactly d_rows_out[0, kept), d_keys_out[0, 29 kept),
 * d_range_off_out[0, m + 1), d_total_out[0] and the workspace. Inputs are
 * unchanged; the outputs must not overlap the inputs. With cap == 0 only the
 * m + 1 offsets and the total (all 0) are written.
 * Every index derived from device data is clamped to cap, m, n or v: pos,
 * range, an offset of d_range_off or d_obj_off, d_latest[j]. Garbage there
 * may give wrong rows, never an access outside the arrays or a search that
 * does not end.
 * d_work is honu_key_filter_workspace(cap) bytes, 256-byte aligned (unused,
 * and NULL allowed, when that is 0). The kept counts of the tiles, one per
 * "filter_tile" rows, are summed by the context's scan (the one behind
 * honu_exclusive_scan), whose state covers honu_ctx_max_records rows: cap may
 * be up to "filter_tile" * honu_ctx_max_records (1024 rows per record the
 * context was created for), and one context serves one stream at a time, as
 * for honu_key_list and honu_key_delete. Asynchronous on `stream`, no host
 * synchronisation, no allocation; the grid is sized from cap, never from a
 * count on the device; replays from a captured graph, also after d_total, the
 * rows or the info were changed on the device between replays.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for cap, m or n above 2^32
 * - 1, or for cap above "filter_tile" * honu_ctx_max_records (more tiles than
 * the context's scan covers); HONU_E_ARG for a NULL ctx, d_range_off, d_total,
 * d_range_off_out or d_total_out, a NULL d_rows or d_rows_out with cap > 0,
 * HONU_FILTER_DELETED without all of d_valid, d_obj_off, d_latest, d_objects
 * and d_info, one of d_keys and d_keys_out without the other, unknown flag
 * bits, d_rows_out == d_rows, d_range_off_out == d_range_off, d_total_out ==
 * d_total or d_keys_out == d_keys, work_bytes below
 * honu_key_filter_workspace(cap), a NULL or misaligned (256) workspace when
 * that size is not 0, or a misaligned pointer (4 bytes: d_latest; 8 bytes:
 * d_range_off, d_total, d_valid, d_obj_off, d_objects, d_info,
 * d_range_off_out, d_total_out; 16 bytes: d_rows, d_rows_out).
 * The get-only param "filter_tile" is the list rows one workgroup takes. */
int32_t honu_key_filter(honu_ctx *ctx, const honu_list_row *d_rows,
                        const uint8_t *d_keys /* optional, 29 B per row */,
                        const uint64_t *d_range_off, uint64_t m, const uint64_t *d_total,
                        uint64_t cap, uint32_t flags,
                        /* HONU_FILTER_DELETED only: */
                        const uint64_t *d_valid, uint64_t n, const uint64_t *d_obj_off,
                        const uint32_t *d_latest, const uint64_t *d_objects,
                        const honu_record_info *d_info,
                        honu_list_row *d_rows_out, uint8_t *d_keys_out, uint64_t *d_range_off_out,
                        uint64_t *d_total_out, void *d_work, uint64_t work_bytes, void *stream);

/* honu_key_next ops: which of Collection's writes the batch is (one per call) */
enum {
    HONU_NEXT_CREATE = 0, /* Collection.Create, collection.go:75-95 */
    HONU_NEXT_UPDATE = 1, /* Collection.Update, collection.go:112-121 */
    HONU_NEXT_MERGE  = 2, /* Collection.Merge ("upsert"), collection.go:123-130 */
    HONU_NEXT_DELETE = 3  /* Collection.Delete, collection.go:132-137; Tombstone(), metadata/collection.go:56-63 */
};

/* honu_next.flags */
enum {
    HONU_NEXT_ASSIGNED   = 1u << 0, /* the request writes a version: vid, pid and the key are set */
    HONU_NEXT_HAS_PARENT = 1u << 1, /* ASSIGNED and Version.Parent != nil: parent_vid, parent_pid */
    HONU_NEXT_TOMBSTONE  = 1u << 2, /* ASSIGNED by HONU_NEXT_DELETE: the version is a tombstone */
    HONU_NEXT_FOUND      = 1u << 3, /* the column holds a version of the object: Collection.Has, collection.go:47-51 */
    HONU_NEXT_LIVE       = 1u << 4, /* FOUND and, with d_order and d_info, the stored latest version is no
                                       tombstone: Exists AS DOCUMENTED (collection.go:53-54), HONU_SEEK_LATEST_LIVE */
    HONU_NEXT_NOT_FOUND  = 1u << 5, /* UPDATE, DELETE: not ASSIGNED, there is no live object to write to */
    HONU_NEXT_EXISTS     = 1u << 6, /* CREATE: not ASSIGNED, the object is stored or an earlier request made it */
    HONU_NEXT_BAD_KEY    = 1u << 7, /* byte 0 of the request is not keyVersion: Key.Check, keys.go:110-120 */
    HONU_NEXT_SKIPPED    = 1u << 8, /* d_req_status[i] != HONU_OK: not looked up */
    HONU_NEXT_WRAPPED    = 1u << 9  /* ASSIGNED and the VID passed 2^64 - 1 (Go's uint64 wraps the same way) */
};

/* One result row of honu_key_next per request. */
typedef struct honu_next {
    uint64_t vid;           /* Version.Scalar.VID */
    uint64_t parent_vid;    /* Version.Parent.VID (HAS_PARENT) */
    uint32_t pid;           /* Version.Scalar.PID */
    uint32_t parent_pid;    /* Version.Parent.PID (HAS_PARENT) */
    uint32_t parent_record; /* d_order[end - 1] when the parent is the stored latest row and d_order is
                               given, else HONU_SEEK_NONE */
    uint32_t flags;         /* HONU_NEXT_* */
} honu_next;                /* 32 */
uint64_t honu_sizeof_next(void);

/* Bytes of honu_key_next's workspace for m requests: the sort's workspace for
 * m keys plus the packed requests, their sorted column, the order, the status
 * column and the count. A multiple of 256, monotonic in m, 0 for m == 0; needs
 * no device. */
uint64_t honu_key_next_workspace(uint64_t m);

/* The version each of a batch of writes writes: the step between a caller's
 * honu_meta rows and honu_encode*, and between its object IDs and
 * honu_sort_keys -> honu_key_merge. Every write of the reference first decides
 * its version: Store.Drop seeks the stored version and calls
 * meta.Tombstone(lamport.ProcessID(), region) (store.go:361-395), which is
 * pid.Next(&c.Version.Scalar) with the stored scalar as Parent
 * (metadata/collection.go:56-63, lamport/pid.go:10-15); Store.New and
 * Collection.Create start a history at Scalar{PID: 0, VID: 1}
 * (store.go:192-198, collection.go:87-92). The bodies of Collection.Update,
 * Merge, Delete and Retrieve are stubs upstream: the ops below are their doc
 * comments (collection.go:112-137: "create a new version record ... if the
 * object does not already exist, it will return an error", "upsert", "adding
 * a tombstone version") carried out with the code of Drop, New, Create and
 * Tombstone. honu_amd/keys.py next() is the host statement; this call equals
 * it bit for bit.
 * Requests. d_requests holds m 29-byte rows of which only bytes [0, 17) are
 * read, the ObjectPrefix (keys.go:74-79): keyVersion | ObjectID. A request
 * with d_req_status[i] != HONU_OK (d_req_status may be NULL) is not looked at
 * and gets SKIPPED alone; any other request whose byte 0 is not 0x01 gets
 * BAD_KEY alone. Neither counts in a rank.
 * What is looked up for every other request: its object's rows [pos, end) of
 * the column (d_sorted, v = min(d_valid[0], n) rows, read on the device), the
 * seek of a 17-byte probe as honu_key_seek defines it, without ObjectLimit's
 * wrap; FOUND = pos < end; the stored latest scalar (P, V) = BE32 of bytes
 * [25, 29) and BE64 of bytes [17, 25) of row end - 1; LIVE = FOUND without
 * d_info (Has), FOUND && !d_info[d_order[end - 1]].tombstone with d_order and
 * d_info (an index not below n reads info row n - 1, as honu_key_seek: d_info
 * is indexed by record and clamped by the column's rows, so LIVE answers for
 * the column only while every index in its valid rows is below n; over a view
 * of a bucketed column see honu_key_merge_buckets, "d_info over a view"); and
 * its rank r, the number of earlier requests of this call, in request order,
 * that count and have the same 17 bytes. FOUND and LIVE report the column as
 * it is stored, whatever earlier requests do to the object.
 * The call then answers as the Go calls would one after the other (VIDs are
 * uint64 and wrap as Go's; an ASSIGNED row with V + 1 + r > 2^64 - 1 also
 * carries WRAPPED):
 *   CREATE  ASSIGNED when !FOUND && r == 0: Scalar {0, 1} (collection.go:88:
 *           not the process's PID), no parent. Otherwise EXISTS.
 *   UPDATE  ASSIGNED when LIVE: Scalar {pid, V + 1 + r}; Parent {P, V} for r ==
 *           0, the stored row, else {pid, V + r}, the request before it.
 *           Otherwise NOT_FOUND.
 *   MERGE   always ASSIGNED. FOUND (a deleted object too): as UPDATE. Not
 *           FOUND: Scalar {pid, 1 + r} (pid.Next(nil), pid_test.go:12), no
 *           parent for r == 0, else Parent {pid, r}.
 *   DELETE  ASSIGNED when LIVE && r == 0: Scalar {pid, V + 1}, Parent {P, V},
 *           TOMBSTONE. Otherwise NOT_FOUND (a second Delete meets a deleted
 *           object).
 * Outputs, by request. d_out[i]: the row above; a row that is not ASSIGNED has
 * vid, pid, parent_vid and parent_pid 0 and parent_record HONU_SEEK_NONE, and
 * so has the parent of an ASSIGNED row without HAS_PARENT. d_keys_out + 29 i
 * (any byte alignment): keys.New (keys.go:42-51) of the request's ObjectID and
 * the assigned scalar for an ASSIGNED row, else the request's 17 bytes and 12
 * zero bytes. d_key_status[i]: HONU_OK for an ASSIGNED row, else
 * HONU_ERR_INPUT. d_keys_out and d_key_status are honu_sort_keys' input as
 * they stand, so next -> sort -> merge runs on one stream with no host read.
 * d_meta (optional; m honu_meta rows, in and out) takes the stamping Create
 * describes ("the metadata pointer will be modified to include the assigned
 * version and ID, and timestamps", collection.go:81-92). Only ASSIGNED rows
 * are touched, and of them only vid, pid, parent_pid, parent_vid (0 without a
 * parent), tombstone (1 for DELETE, else 0), region, version_created = now,
 * modified = now, created = now where there is no parent, object_id =
 * request[1, 17), and in `present` HONU_HAS_META | HONU_HAS_VERSION set and
 * HONU_HAS_PARENT set or cleared. Every other byte of every row stays as it
 * was. A tombstone's other fields are not cleared (upstream does that for
 * collections only); the caller encodes the row with an empty payload, which
 * is what Object.Tombstone() reads.
 * The write set is exactly d_out[0, m), d_keys_out[0, 29 m), d_key_status[0,
 * m), the named fields of d_meta and the workspace. Inputs are unchanged; the
 * outputs must not overlap the inputs. With m == 0 nothing is launched or
 * stored. Every index read from device memory is clamped to n, v or m: garbage
 * in d_valid, d_order or the column may give wrong rows, never an access
 * outside the arrays or a search that does not end.
 * d_work is honu_key_next_workspace(m) bytes, 256-byte aligned (NULL allowed
 * when that is 0). The requests are sorted with the context's scan state
 * (the one behind honu_exclusive_scan): m <= honu_ctx_max_records, and one
 * context serves one stream at a time, as for honu_sort_keys. Asynchronous on
 * `stream`, no host synchronisation, no allocation; the grids are sized from
 * m; replays from a captured graph, also after d_valid, the column or the
 * requests were changed on the device between replays.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for m above
 * honu_ctx_max_records, or n or m above 2^32 - 1; HONU_E_ARG for a NULL ctx or
 * d_valid, a NULL d_sorted with n > 0, a NULL d_requests, d_out, d_keys_out or
 * d_key_status with m > 0, an unknown op, d_info without d_order, d_keys_out
 * == d_requests, work_bytes below honu_key_next_workspace(m), a NULL or
 * misaligned (256) workspace when that size is not 0, or a misaligned pointer
 * (4 bytes: d_order, d_req_status, d_key_status; 8 bytes: d_out, d_valid,
 * d_info, d_meta). */
int32_t honu_key_next(honu_ctx *ctx, const uint8_t *d_sorted, const uint64_t *d_valid, uint64_t n,
                      const uint32_t *d_order /* optional */, const honu_record_info *d_info /* optional */,
                      const uint8_t *d_requests, const int32_t *d_req_status /* optional */, uint64_t m,
                      uint32_t op, uint32_t pid, uint32_t region, int64_t now,
                      honu_next *d_out, uint8_t *d_keys_out, int32_t *d_key_status,
                      honu_meta *d_meta /* optional */, void *d_work, uint64_t work_bytes, void *stream);

/* honu_seek.flags of a row honu_key_compare wrote, beside HONU_SEEK_FOUND: above
 * bit 7, so the seek bits keep their meaning. Exactly one of LATER, EARLIER and
 * EQUAL is set. */
enum {
    HONU_CMP_PEER_HAS = 1u << 8,  /* the peer's column holds a row of the object: b0 < b1 */
    HONU_CMP_LATER    = 1u << 9,  /* lamport.Compare(my latest, the peer's latest) > 0, or the peer has none */
    HONU_CMP_EARLIER  = 1u << 10, /* lamport.Compare(my latest, the peer's latest) < 0 */
    HONU_CMP_EQUAL    = 1u << 11, /* both hold the same latest version */
    HONU_CMP_ANCESTOR = 1u << 12  /* PEER_HAS and the older side's latest key is a row of the newer side:
                                     no fork. PEER_HAS without it is the branch of collection.go:77-79 */
};

/* Bytes of honu_key_compare's workspace for na rows of A: the tiles' class
 * counts. A multiple of 256, monotonic in na, 0 for na == 0; needs no device. */
uint64_t honu_key_compare_workspace(uint64_t na);

/* The versions of two sorted key columns compared object by object: what two
 * replicas decide when they meet. A lamport.Scalar "uses a 'latest writer
 * wins' policy to determine how to solve conflicts" (lamport/scalar.go:15-24),
 * lamport.Compare is the happens-before test (scalar.go:47-78), and a key
 * stores the version big endian "to maintain lexicographic sorting"
 * (keys/keys.go:35-36), so bytes.Compare of two keys of one object is
 * lamport.Compare of their versions. Iterator.Object() "is also used for
 * replication" (iterator/iterator.go:19-23); Collection.Create promises that
 * "branches can be detected later" (collection.go:77-79). honu_amd/keys.py
 * compare() is the host statement; this call equals it.
 * Inputs. A is the local column, B the peer's: each what honu_sort_keys,
 * honu_key_merge or honu_key_delete writes, 29-byte rows at any byte
 * alignment, the valid rows [0, v), v = min(d_valid[0], n), read on the
 * device. B may be the peer's whole column or a digest of it, one key per
 * object, the peer's latest: only the last row of an object's range in B
 * decides the class. A's objects are what honu_key_objects wrote for it
 * (d_obj_off_a, na + 1 values readable; d_objects_a): objects =
 * min(d_objects_a[0], na), and every offset is clamped to va.
 * For object j of A let [a0, a1) be its rows, K = A[a1 - 1] its latest key and
 * [b0, b1) the rows of B whose first 17 bytes are K's: prefix equality, not
 * ObjectLimit's wrapping limit[16]++ (keys.go:88-91), as in honu_key_objects
 * and honu_key_seek. d_out[j] is one honu_seek row, so honu_key_list takes
 * d_out as its d_ranges (it reads pos, end and SKIPPED only; with m = na,
 * which is all the host knows, the caller clears d_out before the call, so
 * that the rows from `objects` on are empty ranges):
 *   end     a1.
 *   pos     with b0 < b1 the first row of [a0, a1) whose key is greater than
 *           B[b1 - 1] over all 29 bytes (the upper bound), else a0. [pos, end)
 *           are my versions later than anything the peer holds, what
 *           latest-writer-wins sends; empty for an object that is equal or
 *           behind.
 *   first, latest  d_order_a[pos], d_order_a[end - 1] when d_order_a is given
 *           and pos < end, else HONU_SEEK_NONE.
 *   flags   HONU_SEEK_FOUND when pos < end; HONU_CMP_PEER_HAS when b0 < b1;
 *           one of HONU_CMP_LATER (K above B[b1 - 1], or the peer has none),
 *           HONU_CMP_EARLIER and HONU_CMP_EQUAL; HONU_CMP_ANCESTOR, with
 *           PEER_HAS only: for LATER pos > a0 and A[pos - 1] == B[b1 - 1], for
 *           EARLIER K is a row of B[b0, b1), for EQUAL always. PEER_HAS
 *           without ANCESTOR is a forked write. For EARLIER that is meaningful
 *           only when B is the peer's whole column: a digest holds no older
 *           row to find K among, so every EARLIER object of a digest reads as
 *           a fork. HONU_SEEK_SKIPPED is never set, nor any other seek bit.
 * Equal keys form runs, as after a merge; the bounds above say which row of a
 * run counts. An object whose rows are empty after the clamps (garbage
 * offsets alone) gets pos = end = a1 and, when a1 is 0, no flag at all.
 * d_peer (optional, room for na): d_peer[j] = b1 - 1, the peer's latest row,
 * or HONU_SEEK_NONE without PEER_HAS. d_counts (optional, 8 values): objects
 * compared; only mine (no PEER_HAS); LATER with PEER_HAS; EARLIER; EQUAL;
 * forks (PEER_HAS without ANCESTOR); 0; 0. The sums are made without atomics
 * and are the same every time. The objects only the peer has are the "only
 * mine" rows of the call with the sides exchanged; there is no second mode.
 * The exact per-key difference A \ B is honu_key_delete(A, B, 29).
 * The write set is exactly d_out[0, objects), d_peer[0, objects), d_counts[0,
 * 8) and the workspace. With na == 0 only d_counts (zeros) is written. Inputs
 * are unchanged. Garbage in d_obj_off_a, d_objects_a or the valid counts may
 * give wrong rows, never an access outside the na / nb rows or a search that
 * does not end; pos <= end <= va always holds.
 * d_work is honu_key_compare_workspace(na) bytes, 256-byte aligned (NULL
 * allowed when that is 0). No use of the context's scan state: calls on
 * different streams may share a context, as with honu_key_seek and
 * honu_key_merge. Asynchronous on `stream`, no host synchronisation, no
 * allocation; the grid is sized from na; replays from a captured graph, also
 * after the counts were changed on the device between replays.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for na or nb above 2^32 -
 * 1; HONU_E_ARG for a NULL ctx, d_valid_a, d_valid_b, d_obj_off_a or
 * d_objects_a, a NULL d_sorted_a with na > 0 or d_sorted_b with nb > 0, a NULL
 * d_out with na > 0, work_bytes below honu_key_compare_workspace(na), a NULL
 * or misaligned (256) workspace when that size is not 0, or a misaligned
 * pointer (4 bytes: d_out, d_peer, d_order_a; 8 bytes: d_counts, d_valid_a,
 * d_valid_b, d_obj_off_a, d_objects_a).
 * The get-only params "compare_tile" and "compare_stage" are the objects one
 * workgroup takes and the rows of B it stages in LDS at most. */
int32_t honu_key_compare(honu_ctx *ctx, const uint8_t *d_sorted_a, const uint32_t *d_order_a /* optional */,
                         const uint64_t *d_valid_a, uint64_t na,
                         const uint64_t *d_obj_off_a, const uint64_t *d_objects_a,
                         const uint8_t *d_sorted_b, const uint64_t *d_valid_b, uint64_t nb,
                         honu_seek *d_out, uint32_t *d_peer /* optional */, uint64_t *d_counts /* optional */,
                         void *d_work, uint64_t work_bytes, void *stream);

/* Bytes of honu_key_reclaim's workspace for nrec records: the marks, the
 * tiles' keep masks and counts and a remap. A multiple of 256, monotonic in
 * nrec, 0 for nrec == 0, at most 8 nrec + 2^20; needs no device. */
uint64_t honu_key_reclaim_workspace(uint64_t nrec);

/* The space a Drop frees. Store.Drop exists "to free up space in the
 * database" (store.go:314-322), and after the DeleteBucket behind it bbolt
 * "marks the pages as free" (store.go:399-404). honu_key_delete compacts the
 * 29-byte column alone; this call compacts what the column's d_order indexes:
 * the records arena with its offsets, and the per-record arrays a resident
 * store keeps beside it (the unsorted keys, their statuses, the
 * honu_record_info rows), to the records the column still names, and rewrites
 * the order to the new indices. honu_amd/keys.py reclaim() is the host
 * statement; this call equals it.
 * Inputs. d_order, d_valid and n are the column's order as honu_sort_keys,
 * honu_key_merge or honu_key_delete wrote it: v = min(d_valid[0], n) is read
 * on the device. The sorted column itself is not an argument: its first v rows
 * stand as they are. d_rec, d_rec_off[nrec + 1] are the records arena (any
 * byte alignment), rec_bytes its readable size. d_keys (29-byte rows, any
 * byte alignment), d_key_status and d_info are optional, each indexed by
 * record, nrec rows; each is given exactly when its output is.
 * Kept records. Record r < nrec is kept when d_order[p] == r for some p < v.
 * The kept records are renumbered 0 .. kept - 1 in ascending old index, new(r):
 * a stable renumbering, so arrival order survives, on which b_base, the
 * merge's tie rule and HONU_DELETE_SUPERSEDED rest. Records named only by
 * rows at or past v are freed: the removed rows of a delete, the invalid rows
 * of a batch.
 * Outputs. d_kept[0] = kept. d_source[j], j < kept, is the old index of new
 * record j (room for nrec): a caller gathers per-record arrays of its own with
 * it. d_remap[r] (optional), every r < nrec, is new(r) or HONU_SEEK_NONE.
 * d_order_out[p] is new(d_order[p]) for p < v, HONU_SEEK_NONE when d_order[p]
 * >= nrec, and HONU_SEEK_NONE for v <= p < n: all n entries are written.
 * d_keys_out row j is the 29 bytes of d_keys row d_source[j];
 * d_key_status_out[j] and d_info_out[j] likewise, the info row verbatim, so
 * its data_off stays relative to the batch it was decoded from.
 * Lengths follow honu_key_fetch: with r = d_source[j], a = d_rec_off[r] and b
 * = d_rec_off[r + 1] give length b - a and d_status[j] (optional, room for
 * nrec) = HONU_OK when a <= b <= rec_bytes, else length 0 and HONU_ERR_INPUT.
 * d_rec_off_out[0, nrec] is the exclusive scan of the lengths, the entries at
 * or past kept counting 0: flat at the total from kept on, and d_val_total[0]
 * is that total. New record j is copied to d_values + d_rec_off_out[j] exactly
 * when its length is not 0 and d_rec_off_out[j + 1] <= val_cap: the fetch's
 * prefix rule, and a caller that reads d_val_total[0] > val_cap re-issues with
 * more room. d_values may be NULL only with val_cap == 0: a sizing call.
 * The write set is exactly d_kept[0], d_val_total[0], d_order_out[0, n),
 * d_remap[0, nrec), d_source[0, kept), rows [0, kept) of the three gathered
 * arrays, d_status[0, kept), d_rec_off_out[0, nrec + 1) and the bytes of the
 * copied records, besides the workspace; the outputs must not overlap the
 * inputs. With nrec == 0 only the two counts (0), d_rec_off_out[0] = 0 and
 * d_order_out[0, n) (all HONU_SEEK_NONE) are written.
 * Garbage in. An index repeated in d_order[0, v) keeps its record once, and
 * both positions get the same new index; a count above n is clamped; an index
 * not below nrec never reads d_rec_off or a per-record row. No record byte
 * outside [0, rec_bytes) is read and no byte outside the write set is written
 * (the copy loads whole aligned 16-byte blocks that hold at least one byte of
 * a record it copies, as every payload copy does).
 * What the result is fit for. With n' = nrec' = kept (the column's first kept
 * rows and d_order_out's first kept entries; after a delete, v == kept of that
 * delete when every kept row names a distinct record), the new state is fit
 * for honu_key_seek, honu_key_objects, honu_key_list, honu_key_fetch,
 * honu_key_filter, honu_key_next, honu_key_compare, a further honu_key_delete
 * and honu_key_merge. A merge after a reclaim needs b_base = kept, and b_base
 * is a host argument: one read of d_kept[0] follows a reclaim, as a caller
 * reads a batch's byte total to size its arena.
 * d_work is honu_key_reclaim_workspace(nrec) bytes, 256-byte aligned (unused,
 * and NULL allowed, when that is 0). The tiles' counts and the nrec + 1
 * lengths are summed by the context's scan, whose state covers max_records
 * rows, so one context serves one stream at a time, as for honu_key_fetch;
 * the copy takes a line of the context's copy counters like every payload
 * copy. Asynchronous on `stream`, no host synchronisation, no allocation; the
 * grids are sized from n and nrec; replays from a captured graph, also after
 * d_valid and d_order were changed on the device between replays.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for n or nrec above 2^32 -
 * 1, or for nrec + 1 above honu_ctx_max_records (honu_key_fetch refuses cap +
 * 1 the same way); HONU_E_ARG for a NULL ctx, d_valid, d_kept, d_val_total,
 * d_rec_off, d_rec_off_out or d_source, a NULL d_order or d_order_out with n >
 * 0, a NULL d_rec with rec_bytes > 0, a NULL d_values with val_cap > 0, an
 * optional input without its output or the output without its input, flags
 * other than 0, work_bytes below honu_key_reclaim_workspace(nrec), a NULL or
 * misaligned (256) workspace when that size is not 0, or a misaligned pointer
 * (4 bytes: the orders, d_remap, d_source, the statuses; 8 bytes: the counts,
 * the offsets, the info rows).
 * The get-only param "reclaim_tile" is the records one workgroup takes. */
int32_t honu_key_reclaim(honu_ctx *ctx, const uint32_t *d_order, const uint64_t *d_valid, uint64_t n,
                         const uint8_t *d_keys /* optional */, const int32_t *d_key_status /* optional */,
                         const honu_record_info *d_info /* optional */,
                         const uint8_t *d_rec, const uint64_t *d_rec_off, uint64_t nrec, uint64_t rec_bytes,
                         uint32_t flags,
                         uint32_t *d_order_out, uint32_t *d_remap /* optional */, uint32_t *d_source,
                         uint8_t *d_keys_out, int32_t *d_key_status_out, honu_record_info *d_info_out,
                         uint64_t *d_rec_off_out, int32_t *d_status /* optional */,
                         uint8_t *d_values, uint64_t val_cap, uint64_t *d_kept, uint64_t *d_val_total,
                         void *d_work, uint64_t work_bytes, void *stream);

/* Bytes of honu_key_route's workspace for a batch of m positions: the packed
 * classes, their sorted column, the order and honu_sort_keys' own workspace. A
 * multiple of 256, monotonic in m, 0 for m == 0; needs no device. */
uint64_t honu_key_route_workspace(uint64_t m);

/* A batch taken apart by collection. Every call above works on one sorted
 * 29-byte column, one bbolt bucket. The reference store has one bucket per
 * collection, named by the 16-byte collection ID:
 * tx.CreateBucketIfNotExists(info.ID[:]) (store.go:236-240);
 * t.tx.Bucket(collectionID[:]), where a nil bucket is ErrRepairCollection
 * (tx.go:112-120); Tx.Has(collection, id) and Tx.Exists(collection, id)
 * (tx.go:141-158). Every object carries the collection it belongs to
 * (meta.CollectionID = c.ID, collection.go:86; honu_meta.collection_id, offset
 * 112). A marshalled batch, a write-feed slot or the batch that
 * honu_key_compare -> honu_key_list -> honu_key_fetch ships to a peer holds
 * records of many collections mixed together; this call looks every record's
 * collection ID up in the store's table of collections and partitions the
 * batch stably by the bucket found. honu_amd/keys.py route() is the host
 * statement; this call equals it.
 * Inputs. Record i's collection ID is the 16 bytes at d_ids + id_stride * i,
 * i < m; d_ids may have any byte alignment, id_stride >= 16. (const uint8_t
 * *)d_meta + 112 with stride 352 makes the decoded rows the input as they
 * stand; stride 16 takes a packed ID column, for example the collection
 * column of a batch of Tx.Has(collection, id) probes. d_status (optional, m
 * values): record i takes part when d_status is NULL or d_status[i] ==
 * HONU_OK. d_table is the store's collections: k rows of 16 bytes at any byte
 * alignment, ascending by bytes.Compare and distinct, the sorted list of
 * bucket names. d_keys (optional, 29 m bytes, any byte alignment) is the
 * batch's key column, by record.
 * Sequence. Position p < m stands for record i = d_seq[p], or i = p without
 * d_seq. With d_seq the order honu_sort_keys wrote for this batch's keys and
 * d_status the status column that sort was given, each bucket's rows come out
 * in key order, equal keys in arrival order: a stable partition of a sorted
 * sequence leaves every part sorted, which is exactly what honu_sort_keys
 * would have returned for that collection's records alone. One sort and one
 * route replace k sorts, and each segment is, as it stands, the B side of a
 * honu_key_merge into that collection's column.
 * Classes. Each position gets a class c: c < k when the record takes part
 * and row c of d_table equals its ID (on garbage, the first such row the
 * search meets); c = k when it takes part and no row equals its ID, the nil
 * bucket of tx.go:117-120; c = k + 1 when the record does not take part
 * (status not HONU_OK) or d_seq[p] >= m, which names no record.
 * Outputs. Output row g is the g-th position when the positions are ordered
 * by (class, p): a stable partition. d_bucket_off[c], c in [0, k + 2], is the
 * first row of class c, d_bucket_off[k + 2] = m, and d_bucket_count[c] =
 * d_bucket_off[c + 1] - d_bucket_off[c], c in [0, k + 1]. d_bucket_off + k is
 * therefore a valid d_total for honu_key_fetch (the routed rows), and
 * d_bucket_count + c a valid d_valid_b for honu_key_merge.
 * d_rows[g] (optional) = {range: c, pos: p, record: i, flags}: record is
 * HONU_SEEK_NONE when d_seq[p] >= m; flags carries HONU_LIST_ROW_HEAD on the
 * first row of every non-empty class, the two tail classes included, and no
 * other bit. The rows are a honu_list_row list: honu_key_fetch gathers the
 * records bucket by bucket with nothing read on the host.
 * d_local[g] (optional) = g - d_bucket_off[c]: the record's index inside its
 * collection's segment once gathered, that is, honu_key_merge's d_order_b.
 * d_keys_out + 29 g (optional) is the 29 bytes of d_keys row i, moved as
 * bytes and never a byte past them, 29 zero bytes when the position names no
 * record; it is given together with d_keys and not without it.
 * d_bucket[i] (optional) = c for c < k, else HONU_SEEK_NONE, written for
 * every i some position names: every record when d_seq is a permutation or
 * absent. It answers a batch of Tx.Has / Tx.Exists probes' bucket lookups.
 * The write set is exactly d_bucket_off[0, k + 3), d_bucket_count[0, k + 2),
 * d_rows[0, m), d_local[0, m), d_keys_out[0, 29 m) and the named d_bucket
 * entries, besides the workspace. With m == 0 only the offsets and counts are
 * written, all zero.
 * Garbage in. A table out of order or with repeats, or a d_seq that is no
 * permutation, may give wrong classes or rows. It never gives an access
 * outside the arrays or a search that does not end: a table row asked lies
 * in [0, k), a record read is below m, and every bisection's bracket shrinks
 * at each step.
 * What follows the call. honu_key_merge's nb and the segments' pointers are
 * host arguments, so one host read of d_bucket_off follows a route, as one
 * read of d_kept follows a reclaim and a caller reads a batch's byte total to
 * size its arena. honu_key_merge_buckets (below) takes the offsets on the
 * device and needs no such read.
 * d_work is honu_key_route_workspace(m) bytes, 256-byte aligned (unused, and
 * NULL allowed, when that is 0). Three steps on `stream`: the classes, a
 * honu_sort_keys over them with the context's scan state (whose state covers
 * max_records rows, hence m <= honu_ctx_max_records, and one context serves
 * one stream at a time), the rows and offsets. Asynchronous on `stream`, no
 * host synchronisation, no allocation; the grids are sized from m and k;
 * replays from a captured graph, also after the IDs, the statuses and the
 * table's bytes were changed on the device between replays.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for m above
 * honu_ctx_max_records or 2^32 - 1, or k above 2^32 - 4; HONU_E_ARG for a
 * NULL ctx, d_bucket_off or d_bucket_count, a NULL d_ids with m > 0,
 * id_stride below 16, a NULL d_table with k > 0, exactly one of d_keys and
 * d_keys_out, work_bytes below honu_key_route_workspace(m), a NULL or
 * misaligned (256) workspace with m > 0, or a misaligned pointer (4 bytes:
 * d_status, d_seq, d_bucket, d_local; 8 bytes: the offsets and counts; 16
 * bytes: d_rows).
 * The get-only param "route_stage" is the table rows a workgroup stages in
 * LDS at most; a longer table is searched in global memory, with the same
 * classes. */
int32_t honu_key_route(honu_ctx *ctx, const uint8_t *d_ids, uint64_t id_stride,
                       const int32_t *d_status /* optional */, uint64_t m,
                       const uint32_t *d_seq /* optional */,
                       const uint8_t *d_table, uint64_t k,
                       const uint8_t *d_keys /* optional */,
                       uint32_t *d_bucket /* optional */,
                       honu_list_row *d_rows /* optional */, uint32_t *d_local /* optional */,
                       uint8_t *d_keys_out /* with d_keys */,
                       uint64_t *d_bucket_off, uint64_t *d_bucket_count,
                       void *d_work, uint64_t work_bytes, void *stream);

/* A routed batch merged into every collection's bucket at once: collections.Put
 * (store.go:232, 395, 530) for a whole mixed batch, each record into the bucket
 * tx.Bucket(collectionID[:]) names (store.go:236-240, tx.go:112-120). What k
 * calls of honu_key_merge do after one host read of honu_key_route's
 * d_bucket_off, in one call with nothing read on the host.
 * honu_amd/keys.py merge_buckets() is the host statement; this call equals it.
 * The bucketed column. All k buckets' columns lie end to end in one arena:
 * d_sorted holds 29-byte rows at any byte alignment, d_order one uint32 record
 * index per row, d_off is uint64[k + 1], ascending, d_off[0] = 0. Bucket c is
 * the rows [d_off[c], d_off[c + 1]), sorted by bytes.Compare; it is the bucket
 * named by row c of the store's sorted table of collections (honu_key_route's
 * d_table). An optional d_count (uint64[k]) gives a bucket's valid rows,
 * min(d_count[c], d_off[c + 1] - d_off[c]), its first; without it every row
 * of a bucket is valid. A view (d_sorted + 29 off[c], d_order + off[c],
 * d_count + c, rows) is an input of every per-bucket call above, and a
 * honu_key_delete over a view that writes its d_valid_out into a count array
 * produces the next call's d_count_a.
 * d_info over a view. honu_key_seek, honu_key_list, honu_key_filter and
 * honu_key_next index d_info by record and clamp the index by n, the rows of
 * the column they are given; over a view that is the view's rows. A per-bucket
 * call given d_info therefore answers for a view only while every index in the
 * view's valid rows is below the view's rows; an index at or above them reads
 * info row rows - 1, and nothing signals it. Per-bucket numbering (d_order_b =
 * d_local, d_base the buckets' record counts) keeps the condition while a
 * bucket holds no more records than rows. This call is tight: after a
 * honu_key_delete over a view the next merge squeezes the removed rows out,
 * the bucket then has fewer rows than records, and every later record of it
 * has an index at or above the view's rows. So a delete over a view must be
 * followed by a honu_key_reclaim of that bucket (its view, its d_count entry
 * and its record arrays) before the merge that squeezes it; d_base[c] is then
 * that call's d_kept. The one-numbering form (d_order_b and d_base NULL, a
 * scalar b_base) numbers a bucket's records above its rows from the first
 * batch on and cannot be used with d_info over views. honu_key_objects,
 * honu_key_fetch, honu_key_compare and honu_key_delete take no d_info, and
 * honu_key_reclaim only moves its rows, by record and bounded by nrec: none of
 * them has such a condition.
 * honu_key_route's outputs are a bucketed
 * column as they stand: d_keys_out the rows, d_bucket_off the offsets (its
 * first k + 1 entries are used; the two tail classes lie behind
 * d_bucket_off[k] and reach no bucket), d_local the order.
 * Inputs. A is the resident column (na rows in its arena, d_count_a
 * optional), B the batch (nb rows in its arena: the route's m). na and nb are
 * host bounds; everything else is read on the device. Every offset is clamped
 * to its arena: ea[c] = min(d_off_a[c], na), eb[c] = min(d_off_b[c], nb).
 * Bucket c takes A's first va[c] rows from ea[c], va[c] = min(d_count_a[c],
 * ea[c + 1] - ea[c]) (the whole difference without d_count_a), and all vb[c] =
 * eb[c + 1] - eb[c] rows of B from eb[c].
 * Outputs. d_off_out[0] = 0, d_off_out[c + 1] = d_off_out[c] + va[c] + vb[c]
 * and d_count_out[c] (optional) = va[c] + vb[c]. Output rows [d_off_out[c],
 * d_off_out[c + 1]) are the stable merge of bucket c's valid A rows and its B
 * rows by bytes.Compare: on equal keys every A row before every B row, each
 * side in its own order, the first va[c] + vb[c] rows honu_key_merge writes
 * for those two views. The output is tight: invalid rows of A are dropped, so
 * the call also squeezes what per-bucket deletes left. An A row keeps its
 * index; B's row g of bucket c gets (d_order_b ? d_order_b[g] : g) + (d_base ?
 * d_base[c] : b_base), modulo 2^32. With d_order_b the route's d_local and
 * d_base the buckets' record counts every bucket keeps its own record
 * numbering, exactly k calls of honu_key_merge with b_base = d_base[c]; with
 * both NULL and a scalar b_base the store has one numbering, routed row g
 * being record b_base + g of what honu_key_fetch gathered. d_order_out NULL
 * ignores every order; when given it needs d_order_a whenever na > 0.
 * The write set is exactly d_sorted_out[0, 29 T), d_order_out[0, T) with T =
 * d_off_out[k], d_off_out[0, k + 1) and d_count_out[0, k): nothing at or past
 * row T. The outputs hold na + nb rows and must not overlap the inputs; the
 * caller ping-pongs two arenas, as with honu_key_merge, and sizes them by na +
 * nb, so no host read follows a route. k == 0 writes d_off_out[0] = 0 alone,
 * na + nb == 0 the offsets and counts alone.
 * Garbage in. Offsets that do not ascend, or d_off[0] != 0, may give wrong
 * rows. They never give an access outside the arrays or a search that does
 * not end: every row read lies below na or nb, every offset entry read in
 * [0, k], every output row written below na + nb, and every bracket shrinks
 * at each step.
 * Asynchronous on `stream`, no host synchronisation, no allocation; the grids
 * are sized from na + nb and from k. Without d_count_a the offsets are the sum
 * of two prefix arrays and the call is one launch with no state outside it.
 * With d_count_a the buckets' rows are scanned with the context's scan state
 * (whose state covers max_records rows, hence k + 1 <= honu_ctx_max_records,
 * and one context serves one stream at a time). Replays from a captured graph,
 * also after the offsets, counts and rows were changed on the device.
 * Refusals, each storing nothing: HONU_E_WORKSPACE for na + nb above 2^32 - 1,
 * k above 2^32 - 4, or with d_count_a k + 1 above honu_ctx_max_records;
 * HONU_E_ARG for a NULL ctx, d_off_a, d_off_b or d_off_out, a NULL column with
 * a row count other than 0 (d_sorted_a with na, d_sorted_b with nb,
 * d_sorted_out with na + nb), d_order_out without d_order_a when na > 0,
 * b_base + nb above 2^32 - 1 when d_base is NULL, or a misaligned pointer (4
 * bytes: the orders and d_base; 8 bytes: the offsets and counts).
 * The get-only param "merge_buckets_stage" is the buckets an output tile of
 * "merge_tile" rows touches at most for its slice of offsets to be staged in
 * LDS; above that the slice is searched in global memory, with the same
 * rows. */
int32_t honu_key_merge_buckets(honu_ctx *ctx, uint64_t k,
                               const uint8_t *d_sorted_a, const uint32_t *d_order_a /* optional */,
                               const uint64_t *d_off_a /* k + 1 */,
                               const uint64_t *d_count_a /* optional, k */, uint64_t na,
                               const uint8_t *d_sorted_b, const uint32_t *d_order_b /* optional */,
                               const uint64_t *d_off_b /* k + 1 */, uint64_t nb,
                               const uint32_t *d_base /* optional, k */, uint32_t b_base,
                               uint8_t *d_sorted_out, uint32_t *d_order_out /* optional */,
                               uint64_t *d_off_out /* k + 1 */,
                               uint64_t *d_count_out /* optional, k */, void *stream);

/* ------------------------------------------------------------------------ */
/* System objects (object/system.go): metadata.Collection with its Indexes.  */
/* ------------------------------------------------------------------------ */

/* Presence bit 0 of honu_collection.present: the EncodeStruct flag that
 * MarshalSystem writes for the collection (system.go:22); bits 1-7 as for
 * honu_meta (Version, Parent, Schema, Publisher, Encryption, Compression,
 * non-nil WriteRegions). */
#define HONU_HAS_COLLECTION HONU_HAS_META

/* One metadata.Collection (collection.go:16-33) as a fixed 368-byte row.
 * Field meanings, spans, list descriptors and time encoding as honu_meta;
 * index_off/index_count describe Collection.Indexes in a honu_index table. */
typedef struct honu_collection {
    uint32_t present;            /*   0 HONU_HAS_* bits */
    uint8_t permissions;         /*   4 Collection.Permissions */
    uint8_t flags;               /*   5 Collection.Flags */
    uint8_t tombstone;           /*   6 Version.Tombstone */
    uint8_t compression_alg;     /*   7 */
    uint8_t sealing_alg;         /*   8 */
    uint8_t encryption_alg;      /*   9 */
    uint8_t signature_alg;       /*  10 */
    uint8_t _pad0;               /*  11 */
    uint32_t region;             /*  12 Version.Region */
    uint64_t vid;                /*  16 */
    uint32_t pid;                /*  24 */
    uint32_t parent_pid;         /*  28 */
    uint64_t parent_vid;         /*  32 */
    int64_t version_created;     /*  40 */
    uint32_t schema_major;       /*  48 */
    uint32_t schema_minor;       /*  52 */
    uint32_t schema_patch;       /*  56 */
    uint32_t _pad1;              /*  60 */
    int64_t compression_level;   /*  64 */
    int64_t created;             /*  72 Collection.Created */
    int64_t modified;            /*  80 Collection.Modified */
    uint64_t _pad2;              /*  88 */
    uint8_t id[16];              /*  96 Collection.ID */
    uint8_t owner[16];           /* 112 */
    uint8_t group[16];           /* 128 */
    uint8_t publisher_id[16];    /* 144 */
    uint8_t client_id[16];       /* 160 */
    uint8_t _pad3[16];           /* 176 */
    honu_span name;              /* 192 Collection.Name */
    honu_span schema_name;       /* 208 */
    honu_span ip_address;        /* 224 */
    honu_span user_agent;        /* 240 */
    honu_span public_key_id;     /* 256 */
    honu_span encryption_key;    /* 272 */
    honu_span hmac_secret;       /* 288 */
    honu_span signature;         /* 304 */
    uint64_t acl_off;            /* 320 */
    uint64_t acl_count;          /* 328 len(ACL); 0 <=> nil */
    uint64_t regions_off;        /* 336 */
    uint64_t regions_count;      /* 344 */
    uint64_t index_off;          /* 352 first entry in the index table */
    uint64_t index_count;        /* 360 len(Indexes); 0 <=> nil */
} honu_collection;               /* 368 */

/* One *metadata.Index (index.go:16-22) with its Field / Ref (field.go:12-16).
 * present == 0 is a nil pointer in the Indexes slice. */
typedef struct honu_index {
    uint8_t present;             /*   0 */
    uint8_t type;                /*   1 IndexType */
    uint8_t has_field;           /*   2 Field != nil */
    uint8_t field_type;          /*   3 Field.Type (FieldType) */
    uint8_t has_ref;             /*   4 Ref != nil */
    uint8_t ref_type;            /*   5 Ref.Type */
    uint8_t _pad[10];            /*   6 */
    uint8_t id[16];              /*  16 Index.ID */
    uint8_t field_collection[16];/*  32 Field.Collection */
    uint8_t ref_collection[16];  /*  48 Ref.Collection */
    honu_span name;              /*  64 Index.Name */
    honu_span field_name;        /*  80 Field.Name */
    honu_span ref_name;          /*  96 Ref.Name */
} honu_index;                    /* 112 */

/* ------------------------------------------------------------------------ */
/* System objects on the GPU                                                 */
/* ------------------------------------------------------------------------ */

/* object.MarshalSystem(collection) (system.go:10-31) for n collections:
 * 0x01 | EncodeStruct(collection) | 0x00. Exact encoded lengths in d_sizes,
 * statuses as honu_encode_sizes (HONU_ERR_INPUT for spans or lists outside
 * their arenas). A span is validated only when its struct's presence bit is
 * set, as Go never reads a nil struct's fields; name is always live. A row
 * without HONU_HAS_COLLECTION encodes MarshalSystem(nil) = 01 00 00. d_rows
 * must be 16-byte aligned, d_acl and d_regions 4-byte, d_index 8-byte;
 * d_status may be NULL. */
int32_t honu_system_sizes(honu_ctx *ctx, const honu_collection *d_rows, uint64_t var_len,
                          const honu_acl *d_acl, uint64_t acl_len, const uint32_t *d_regions,
                          uint64_t regions_len, const honu_index *d_index, uint64_t index_len,
                          uint64_t n, uint64_t *d_sizes, int32_t *d_status, void *stream);
/* Writes records at d_out + d_out_off[i] (offsets from honu_exclusive_scan of
 * the sizes); skips records whose status is not HONU_OK, and gives those
 * whose range ends past out_cap HONU_ERR_CAPACITY (nothing of them is
 * stored; the call still returns HONU_OK). d_rows and d_out must be 16-byte
 * aligned, the tables as for honu_system_sizes. */
int32_t honu_system_encode(honu_ctx *ctx, const honu_collection *d_rows, const uint8_t *d_var,
                           const honu_acl *d_acl, const uint32_t *d_regions,
                           const honu_index *d_index, uint64_t n, uint8_t *d_out,
                           uint64_t out_cap, const uint64_t *d_out_off, int32_t *d_status,
                           void *stream);
/* sizes + scan (d_out_off has n+1 entries) + encode. Every argument check of
 * the three (alignments, null pointers, n against max_records:
 * HONU_E_WORKSPACE) is made before the first launch: a refused call has
 * stored nothing. */
int32_t honu_system_marshal_batch(honu_ctx *ctx, const honu_collection *d_rows,
                                  const uint8_t *d_var, uint64_t var_len, const honu_acl *d_acl,
                                  uint64_t acl_len, const uint32_t *d_regions,
                                  uint64_t regions_len, const honu_index *d_index,
                                  uint64_t index_len, uint64_t n, uint8_t *d_out,
                                  uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status,
                                  void *stream);
/* object.UnmarshalSystem(obj, &metadata.Collection{}) (system.go:33-45) for
 * n records: decodes obj[1 : len-1] (the storage version byte is not checked,
 * the trailing nil-metadata byte is not read). Rows as honu_meta decode
 * (spans absolute in the records arena; fields of nil structs zero; a nil
 * collection leaves a zero row). ACL entries, regions and index rows go to
 * the tables (capacities in entries); d_status[i] is the UnmarshalSystem
 * error, HONU_ERR_PANIC for records shorter than 2 bytes (slice bounds) and
 * for counts Go's make() rejects. d_totals (3 u64, device, optional): the
 * ACL entries, regions and indexes the batch needs, whatever the capacities.
 * A record whose lists do not fit a table keeps its row, with the offsets its
 * lists would have had, gets HONU_ERR_CAPACITY in d_status, and none of its
 * entries is stored; the call returns HONU_OK, as honu_decode_batch does (a
 * capacity shows in the statuses and in the totals, never in the return
 * code). d_rec and d_rows must be 16-byte aligned (the decoder loads whole
 * aligned 16-byte blocks relative to d_rec), d_acl and d_regions 4-byte,
 * d_index 8-byte; a table may be NULL only with capacity 0. n above
 * max_records: HONU_E_WORKSPACE. A refused call has stored nothing. */
int32_t honu_system_decode_batch(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                                 uint64_t n, honu_collection *d_rows, int32_t *d_status,
                                 honu_acl *d_acl, uint64_t acl_cap, uint32_t *d_regions,
                                 uint64_t regions_cap, honu_index *d_index, uint64_t index_cap,
                                 uint64_t *d_totals, void *stream);
/* lani.Unmarshal(raw, &metadata.Collection{}) (lani/lani.go:29-33) for n
 * records: Collection.Decode (collection.go:240-356) from byte 0 of each raw
 * value to its end, as the store calls it on the bbolt value of a system
 * object (store.go:367, whose storage-version and struct-flag bytes are then
 * read as the first bytes of the ID). Rows, tables and statuses as
 * honu_system_decode_batch; a row that decodes has HONU_HAS_COLLECTION set
 * (the target is never nil). store.go:155 passes a nil *Collection, on which
 * Collection.Decode always panics (nil dereference, collection.go:242): no
 * batch call is needed to reproduce that. */
int32_t honu_collection_decode_batch(honu_ctx *ctx, const uint8_t *d_rec,
                                     const uint64_t *d_rec_off, uint64_t n,
                                     honu_collection *d_rows, int32_t *d_status, honu_acl *d_acl,
                                     uint64_t acl_cap, uint32_t *d_regions, uint64_t regions_cap,
                                     honu_index *d_index, uint64_t index_cap, uint64_t *d_totals,
                                     void *stream);

/* ------------------------------------------------------------------------ */
/* Read feed: the local-storage read path (iterator/cursor.go:31-38 copies    */
/* each bbolt value; Collection.Exists, collection.go:55-65, asks Tombstone). */
/* Records are appended into pinned host memory; each submitted batch is      */
/* copied to the device, decoded (zero copy) and keyed on its own stream      */
/* while the next batch fills: two slots, so the H2D copy, the kernels and    */
/* the D2H copies of one batch overlap the host filling the other.            */
/* ------------------------------------------------------------------------ */
typedef struct honu_feed honu_feed;

enum {
    HONU_FEED_HEADERS = 1u << 0  /* StorageVersion/Data/Tombstone only (honu_decode_headers) */
};

/* Host views of a decoded batch, valid until the next append/reserve into the
 * same slot (one more submit). Spans in meta rows and info.data_off are
 * absolute offsets into `records` (the batch's pinned arena), so Data() is the
 * subslice records[data_off : data_off + data_len], as in the reference. */
typedef struct honu_feed_result {
    uint64_t n;                       /* records in the batch */
    const uint8_t *records;           /* pinned arena holding the batch's records */
    const uint64_t *rec_off;          /* n + 1 offsets into records */
    const honu_meta *meta;            /* n rows (NULL with HONU_FEED_HEADERS) */
    const honu_record_info *info;     /* n */
    const honu_acl *acl;              /* acl_n entries (never more than the table holds) */
    uint64_t acl_n;
    const uint32_t *regions;          /* regions_n entries (likewise) */
    uint64_t regions_n;
    const uint8_t *keys;              /* 29 * n bytes, Object.Key() (NULL with HEADERS) */
    const int32_t *key_status;        /* n */
    uint64_t acl_needed;              /* entries the batch needed; > acl_n when the table
                                         overflowed (those records: HONU_ERR_CAPACITY) */
    uint64_t regions_needed;
} honu_feed_result;

/* A feed with two slots of batch_records records / batch_bytes bytes each.
 * The decoded ACL / region tables hold batch_bytes/8 + 1024 and
 * batch_bytes/4 + 1024 entries per batch; a batch that needs more reports
 * HONU_ERR_CAPACITY in the meta_status of the records that did not fit. */
honu_feed *honu_feed_create(int device, uint64_t batch_records, uint64_t batch_bytes,
                            uint32_t flags, int32_t *err);
void honu_feed_destroy(honu_feed *feed);
/* Copy one record into the current batch: HONU_ERR_CAPACITY when it does not
 * fit (submit, then append again), HONU_E_ARG when the slot still holds a
 * batch that was submitted but not waited for. */
int32_t honu_feed_append(honu_feed *feed, const uint8_t *rec, uint64_t len);
/* honu_feed_append for records 0..n-1 of a host CSR arena (record i =
 * arena[off[i], off[i+1]): a cursor page), stopping at the first record that
 * does not fit; *appended = records taken. */
int32_t honu_feed_append_batch(honu_feed *feed, const uint8_t *arena, const uint64_t *off,
                               uint64_t n, uint64_t *appended);
/* Reserve len bytes for the next record in pinned memory and return the
 * pointer (the caller writes the record there), or NULL with *err set. */
uint8_t *honu_feed_reserve(honu_feed *feed, uint64_t len, int32_t *err);
/* Records in the current (filling) batch. */
uint64_t honu_feed_pending(const honu_feed *feed);
/* Start decoding the current batch (asynchronous); *ticket identifies it.
 * The other slot becomes the filling one. */
int32_t honu_feed_submit(honu_feed *feed, uint64_t *ticket);
/* Wait for a submitted batch and describe its results. */
int32_t honu_feed_wait(honu_feed *feed, uint64_t ticket, honu_feed_result *out);

/* ------------------------------------------------------------------------ */
/* Write feed: the local-storage write path (a store Put marshals one record */
/* per call today: object.Marshal, object.go:24-45, from store.go:226,530).  */
/* Records (row + the bytes it references + payload) are appended into      */
/* pinned memory; each submitted batch is copied to the device, marshalled   */
/* and copied back on its own stream while the next batch fills (two slots). */
/* ------------------------------------------------------------------------ */
typedef struct honu_put_feed honu_put_feed;

/* Host views of a marshalled batch, valid until the slot is refilled (one
 * more submit). Record i is records[rec_off[i], rec_off[i+1]) when
 * status[i] == HONU_OK (Marshal's []byte); a failed record has an empty range
 * and its error (HONU_ERR_PANIC for Marshal(nil, ...)). */
typedef struct honu_put_result {
    uint64_t n;
    const uint8_t *records;
    const uint64_t *rec_off;  /* n + 1 */
    const int32_t *status;    /* n */
} honu_put_result;

/* A feed with two slots of batch_records records each; batch_bytes bounds a
 * batch's input bytes: the bytes its rows' spans reference + payloads + 20
 * per ACL entry + 4 per region. */
honu_put_feed *honu_put_feed_create(int device, uint64_t batch_records, uint64_t batch_bytes,
                                    int32_t *err);
void honu_put_feed_destroy(honu_put_feed *feed);
/* Append object.Marshal(meta, data) for one record. `row` is the record's
 * honu_meta: its spans index var[0, var_len), acl_off/acl_count index
 * acl[0, acl_len), regions_off/regions_count index regions[0, regions_len)
 * (a caller may pass whole batch tables or the record's own). Only the bytes
 * and entries the row references are copied (spans of absent sub-structs are
 * ignored). HONU_ERR_CAPACITY: the batch is full (submit, then append again);
 * HONU_ERR_INPUT: a span or list lies outside its array (nothing appended);
 * HONU_E_ARG: the filling slot still holds a batch that was not waited for.
 * data == NULL with data_len == 0 is a nil payload (a tombstone). */
int32_t honu_put_feed_append(honu_put_feed *feed, const honu_meta *row, const uint8_t *var,
                             uint64_t var_len, const honu_acl *acl, uint64_t acl_len,
                             const uint32_t *regions, uint64_t regions_len, const uint8_t *data,
                             uint64_t data_len);
/* honu_put_feed_append for records 0..n-1 of a host CSR batch (payload i =
 * payload[payload_off[i], payload_off[i+1])), stopping at the first record
 * that does not go in; *appended = records taken. */
int32_t honu_put_feed_append_batch(honu_put_feed *feed, const honu_meta *rows, uint64_t n,
                                   const uint8_t *var, uint64_t var_len, const honu_acl *acl,
                                   uint64_t acl_len, const uint32_t *regions, uint64_t regions_len,
                                   const uint8_t *payload, const uint64_t *payload_off,
                                   uint64_t *appended);
uint64_t honu_put_feed_pending(const honu_put_feed *feed);
int32_t honu_put_feed_submit(honu_put_feed *feed, uint64_t *ticket);
int32_t honu_put_feed_wait(honu_put_feed *feed, uint64_t ticket, honu_put_result *out);

/* ------------------------------------------------------------------------ */
/* Host memory helpers (pinned buffers for the host<->device path)          */
/* ------------------------------------------------------------------------ */
void *honu_host_alloc(uint64_t bytes);  /* hipHostMalloc, NULL on failure */
void honu_host_free(void *p);
void *honu_device_alloc(uint64_t bytes); /* hipMalloc on the current device */
void honu_device_free(void *p);
int32_t honu_memcpy_h2d(void *d_dst, const void *h_src, uint64_t bytes, void *stream);
int32_t honu_memcpy_d2h(void *h_dst, const void *d_src, uint64_t bytes, void *stream);
int32_t honu_stream_sync(void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HONU_CODEC_H */
