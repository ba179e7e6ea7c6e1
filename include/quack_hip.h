/*
 * quack_hip.h — C ABI of the MI355X-native quACK power-sum engine
 * (libquack_hip.so).
 *
 * This is the drop-in boundary for the `quack` crate's encode/decode path.
 * The reference exposes it as a Rust crate API, not an FFI;
 * each entry point below names the reference call it replaces, and
 * INTEGRATION.md shows the Rust `extern "C"` binding a maintainer adds so
 * sidekick/ and media/ keep compiling against `quack::PowerSumQuackU32`.
 *
 * Conventions
 *   - Plain C types only; every buffer is caller-owned.  No ownership crosses
 *     the ABI except the opaque qk_ctx (create/destroy).
 *   - Every function returns an int status (QK_OK == 0, negative on error)
 *     unless documented otherwise.  No C++ exception crosses the ABI.
 *   - Sketch state is a POD with a flexible array; size it with
 *     qk_u32_size()/qk_u64_size().  Copying the bytes is Clone
 *     (sidekick.rs:203-205).  The state is not internally synchronised
 *     (the reference guards it with a Mutex: sidekick.rs:107).
 *   - "device" functions run hand-written gfx950 kernels.  They never fall
 *     back to the CPU: with no GPU they return QK_E_NO_DEVICE.
 *   - `stream` is a hipStream_t passed as void*; NULL is the HIP null
 *     (legacy default) stream, so work is ordered with the caller's
 *     default-stream work.  "_async" functions only enqueue on that stream.
 *
 * Field and semantics:  p32 = 2^32-5, p64 = 2^64-59; an id is
 * mapped to x = id mod p; S[k-1] = sum_i x_i^k mod p for k = 1..threshold;
 * count is a wrapping u32; last_value is the last inserted (unreduced) id.
 */
#ifndef QUACK_HIP_H
#define QUACK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QK_P32 4294967291u
#define QK_P64 18446744073709551557ull
#define QK_MAX_THRESHOLD 1024u /* largest threshold the device kernels accept */

enum {
    QK_OK = 0,
    QK_E_INVAL = -1,        /* bad argument (null pointer, host pointer where device expected, ...) */
    QK_E_THRESHOLD = -2,    /* threshold 0 on insert/remove, or > QK_MAX_THRESHOLD on device */
    QK_E_MISMATCH = -3,     /* thresholds of two sketches differ (reference panics) */
    QK_E_UNDECODABLE = -4,  /* count > threshold: caller must reset (media_client.rs:258-261) */
    QK_E_CAPACITY = -5,     /* output buffer too small; *n_out holds the required size */
    QK_E_HIP = -6,          /* a HIP runtime call failed */
    QK_E_NO_DEVICE = -7,    /* no usable gfx950 device */
    QK_E_NOMEM = -8,
    QK_E_FORMAT = -9,       /* malformed serialized bytes */
    QK_E_COMM = -10,        /* a collective failed: the communicator is aborted and unusable */
    QK_E_PEER = -11         /* another rank of the communicator failed (its own call reports why) */
};

const char *qk_strerror(int status);
const char *qk_version(void);

/* ------------------------------------------------------------------------
 * Sketch state (PowerSumQuackU32 / PowerSumQuackU64)
 * ---------------------------------------------------------------------- */
typedef struct qk_u32 {
    uint32_t threshold;
    uint32_t count;       /* wrapping */
    uint32_t has_last;    /* Option tag of last_value */
    uint32_t last_value;
    uint32_t power_sums[]; /* threshold entries, canonical (< QK_P32) */
} qk_u32;

typedef struct qk_u64 {
    uint32_t threshold;
    uint32_t count;
    uint32_t has_last;
    uint32_t reserved;
    uint64_t last_value;
    uint64_t power_sums[]; /* threshold entries, canonical (< QK_P64) */
} qk_u64;

size_t qk_u32_size(uint32_t threshold);                 /* bytes of a qk_u32 */
size_t qk_u64_size(uint32_t threshold);

/* PowerSumQuackU32::new(threshold)   — sidekick/src/sidekick.rs:32 */
int qk_u32_init(qk_u32 *q, uint32_t threshold);
int qk_u64_init(qk_u64 *q, uint32_t threshold);

/* ---- host scalar path (per packet; a kernel launch costs more than an
 *      insert, so these never touch the GPU) ---------------------------- */
/* quack.insert(id)                   — sidekick.rs:42, sidekick_multi.rs:82 */
int qk_u32_insert(qk_u32 *q, uint32_t id);
int qk_u64_insert(qk_u64 *q, uint64_t id);
/* my_quack.remove(id)                — media_client.rs:319 */
int qk_u32_remove(qk_u32 *q, uint32_t id);
int qk_u64_remove(qk_u64 *q, uint64_t id);
/* diff_quack.sub_assign(quack)       — media_client.rs:296 (keeps q->last_value) */
int qk_u32_sub_assign(qk_u32 *q, const qk_u32 *rhs);
int qk_u64_sub_assign(qk_u64 *q, const qk_u64 *rhs);
/* union of two disjoint streams, `later` following q in stream order
 * (additivity): sums add, counts add, last from `later`. */
int qk_u32_merge(qk_u32 *q, const qk_u32 *later);
int qk_u64_merge(qk_u64 *q, const qk_u64 *later);
/* diff_quack.to_coeffs()             — media_client.rs:304.
 * Writes d = q->count coefficients c_1..c_d of prod(z - x_missing).
 * d > threshold -> QK_E_UNDECODABLE; cap < d -> QK_E_CAPACITY (*d set). */
int qk_u32_to_coeffs(const qk_u32 *q, uint32_t *coeffs, uint32_t cap, uint32_t *d);
int qk_u64_to_coeffs(const qk_u64 *q, uint64_t *coeffs, uint32_t cap, uint32_t *d);
/* quack::arithmetic::eval(&coeffs, x).value()   — media_client.rs:310.
 * Returns the canonical value of the monic polynomial at x (d == 0 -> 1). */
uint32_t qk_u32_eval(const uint32_t *coeffs, uint32_t d, uint32_t x);
uint64_t qk_u64_eval(const uint64_t *coeffs, uint32_t d, uint64_t x);

/* decode_with_log over a HOST-resident log (the receiver's short logs,
 * media_client.rs:304-313): to_coeffs, then the root test on the CPU; same
 * contract as qk_u32_decode_device (hits = log positions ascending, cut at
 * the first entry equal to diff->last_value when stop_at_last). */
int qk_u32_decode_host(const qk_u32 *diff, const uint32_t *log, size_t n, int stop_at_last, uint64_t *hits,
                       size_t cap, size_t *n_hits);
int qk_u64_decode_host(const qk_u64 *diff, const uint64_t *log, size_t n, int stop_at_last, uint64_t *hits,
                       size_t cap, size_t *n_hits);

/* bincode 1.3 image of the serde-derived struct
 * {power_sums: Vec<ModularInteger>, last_value: Option<T>, count: u32}
 * (sidekick.rs:187, media_client.rs:227; layout [RECALL]). */
size_t qk_u32_serialized_size(const qk_u32 *q);
int qk_u32_serialize(const qk_u32 *q, uint8_t *buf, size_t cap, size_t *len);
/* Reads the threshold from the bytes; *threshold_out lets the caller size q
 * first (call with q == NULL), then qk_*_init(q, threshold) and call again:
 * q->threshold must equal the serialized threshold (else QK_E_MISMATCH and q
 * is untouched). */
int qk_u32_deserialize(const uint8_t *buf, size_t len, qk_u32 *q, uint32_t *threshold_out);
size_t qk_u64_serialized_size(const qk_u64 *q);
int qk_u64_serialize(const qk_u64 *q, uint8_t *buf, size_t cap, size_t *len);
int qk_u64_deserialize(const uint8_t *buf, size_t len, qk_u64 *q, uint32_t *threshold_out);

/* ------------------------------------------------------------------------
 * Device context
 * ---------------------------------------------------------------------- */
typedef struct qk_ctx qk_ctx;

int qk_device_count(int *n);
int qk_ctx_create(int device, qk_ctx **out);
void qk_ctx_destroy(qk_ctx *ctx);
int qk_ctx_synchronize(qk_ctx *ctx, void *stream);
/* When on, every launch of the dominant kernel (encode / root test) is
 * bracketed by hipEvents on its stream; qk_ctx_kernel_stats() waits for them
 * and returns the summed duration and launch count, then resets. */
int qk_ctx_set_profiling(qk_ctx *ctx, int on);
int qk_ctx_kernel_stats(qk_ctx *ctx, double *total_ms, uint64_t *launches);
/* Growing a context's scratch never synchronises the device: grown-out
 * buffers are retired, not freed (hipFree synchronises every stream).
 * qk_ctx_trim frees them — a device-wide synchronisation, so call it when
 * that is acceptable (qk_ctx_destroy does it too). */
int qk_ctx_trim(qk_ctx *ctx);
/* Tuning knobs (0 = automatic): workgroups per launch. */
int qk_ctx_set_grid(qk_ctx *ctx, uint32_t blocks);
/* Knobs of this context that select between live product paths (DESIGN.md
 * §3; the defaults are the product's measured choices — tools/ and the
 * tests set them): "grid_mult" (1..8: static encode grids of that many
 * rounds of resident workgroups), "enc_dyn" (1: the single-pass u32
 * baby-step/giant-step encode hands its ids out in chunks that waves claim,
 * one resident round; 0: the static form), "u32_basis" (1: the u32 t = 31..32
 * encode forms its 32 powers from a nine-power basis, 8 modular products per
 * id, with a table lookup per id for the ids whose lazy products wrap; 2: the same
 * basis with a running minimum of the products instead of the lookup; 0: from
 * the (8,4) baby-step/giant-step grid, 9), "flow_hist" (per-flow batches of at most this many
 * flows are grouped by slot histograms, 0: never), "flow_byslot" (0 the
 * rule, 1 / 2 force the by-slot / by-rank grouping key), "root_test" (0
 * automatic, 1 Horner, 2 root-set scan), "comm_fault" (tests: the k-th
 * collective's payload staging of this context's rank fails once),
 * "comm_delay_ms" (tests: a kernel of that many ms runs before this rank's
 * next RCCL collective, once), "rt_karg" (1: a root-set scan whose set fits
 * the kernel arguments takes them; 0: always by copy).
 * Unknown name or out-of-range value -> QK_E_INVAL. */
int qk_ctx_set_knob(qk_ctx *ctx, const char *name, int64_t value);
/* Shader-clock probe (measurement): one wave on `stream` spins for
 * `microseconds` of wall time and writes d_out[0] = shader-clock ticks
 * (s_memtime) and d_out[1] = 100 MHz ticks (s_memrealtime) elapsed, so the
 * clock is d_out[0] / d_out[1] * 100 MHz.  Launched beside running kernels it
 * reads the clock the chip holds under their load. */
int qk_clock_probe(qk_ctx *ctx, uint32_t microseconds, uint64_t *d_out, void *stream);
/* Pinned host memory for the host-input path: ids written here by the
 * sniffer are DMA'd without a staging copy. */
int qk_host_alloc(size_t bytes, void **out);
int qk_host_free(void *p);

/* ------------------------------------------------------------------------
 * Batch encode — the hot path.  Replaces the per-id loop
 *   for id in ids { quack.insert(id) }   (sidekick.rs:42 under :76-124;
 *   media_client.rs:247-252; quack benchmark_construct) for an id array.
 * ---------------------------------------------------------------------- */
/* Partial vector written by the _async encoders, u64 words:
 *   u32: [S_1..S_t (canonical), n, last_id]            (t + 2 words)
 *   u64: [lo32(S_k), hi32(S_k) for k = 1..t, n, last_id] (2t + 2 words)
 * The first t+1 (u32) / 2t+1 (u64) words of several partials may be summed
 * elementwise as unsigned 64-bit integers (e.g. an RCCL sum-reduce) without
 * overflow for up to 2^27 partials; qk_*_from_partial folds such a sum. */
size_t qk_u32_partial_words(uint32_t threshold);
size_t qk_u64_partial_words(uint32_t threshold);

int qk_u32_encode_device_async(qk_ctx *ctx, const uint32_t *d_ids, size_t n, uint32_t threshold,
                               uint64_t *d_partial, void *stream);
int qk_u64_encode_device_async(qk_ctx *ctx, const uint64_t *d_ids, size_t n, uint32_t threshold,
                               uint64_t *d_partial, void *stream);
/* Fold a (possibly summed) host copy of the partial into q as the stream that
 * follows q: sums and count add; last_value taken from `last` if has_last. */
int qk_u32_merge_partial(qk_u32 *q, const uint64_t *partial, int has_last, uint32_t last);
int qk_u64_merge_partial(qk_u64 *q, const uint64_t *partial, int has_last, uint64_t last);

/* Synchronous: encode device-resident ids and merge them into q (as if
 * inserted in array order after q's existing content). */
int qk_u32_encode_device(qk_ctx *ctx, const uint32_t *d_ids, size_t n, qk_u32 *q, void *stream);
int qk_u64_encode_device(qk_ctx *ctx, const uint64_t *d_ids, size_t n, qk_u64 *q, void *stream);
/* Synchronous: encode HOST-resident ids (the sniffed-packet case): chunked
 * H2D through pinned staging on two streams, overlapped with the kernel. */
int qk_u32_encode_host(qk_ctx *ctx, const uint32_t *h_ids, size_t n, qk_u32 *q);
int qk_u64_encode_host(qk_ctx *ctx, const uint64_t *h_ids, size_t n, qk_u64 *q);

/* ------------------------------------------------------------------------
 * Packet batches: identifier extraction fused in front of the encode
 * (SURVEY.md §8f rank 2).  Replaces the sniff loop of sidekick.rs:76-124 for
 * a batch of captured buffers: per packet, in order,
 *   skip unless sll_pkttype is PACKET_HOST/PACKET_OTHERHOST      (:78-80)
 *   skip unless sll_protocol == htons(ETH_P_IP)                    (:81-84)
 *   skip unless buf[23] == IPPROTO_UDP      (buffer.rs:80-83)      (:85-88)
 *   dst ip buf[30..34] == my_ipv4 -> reset the quACK               (:92-96)
 *   skip unless the capture length == QK_BUFFER_SIZE               (:99-102)
 *   insert the big-endian u32 at byte QK_ID_OFFSET (buffer.rs:99-106)
 * Buffers are `stride`-byte records (the reference reads QK_BUFFER_SIZE = 67
 * bytes per packet) in device memory; meta may be NULL (all packets incoming
 * IPv4 of full length).  my_ipv4 may be NULL (no packet resets).
 * ---------------------------------------------------------------------- */
#define QK_ID_OFFSET 63u
#define QK_BUFFER_SIZE 67u
typedef struct qk_pkt_meta {
    uint8_t pkttype;      /* sockaddr_ll.sll_pkttype */
    uint8_t reserved;
    uint16_t protocol_be; /* sockaddr_ll.sll_protocol (network byte order, as stored) */
    uint32_t len;         /* bytes returned by recvfrom */
} qk_pkt_meta;
typedef struct qk_pkt_stats {
    uint64_t inserted;    /* inserts that reached the final state (after the last reset) */
    uint64_t discarded;   /* inserts wiped by a later reset in the same batch */
    uint64_t resets;
    uint64_t filtered;    /* packets skipped by the filters */
    int64_t last_reset_index; /* -1 if no reset */
} qk_pkt_stats;
int qk_u32_encode_packets_device(qk_ctx *ctx, const uint8_t *d_bufs, size_t n, size_t stride,
                                 const qk_pkt_meta *d_meta, const uint8_t my_ipv4[4], qk_u32 *q,
                                 qk_pkt_stats *stats, void *stream);

/* ------------------------------------------------------------------------
 * Segmented multi-flow encode: one quACK per flow.
 * ---------------------------------------------------------------------- */
/* AddrKey of sidekick_multi.rs:13 / buffer.rs:91-95:
 * [src ip (4), src port (2), dst ip (4), dst port (2)], bytes as on the wire. */
typedef struct qk_flow_key {
    uint8_t addr[12];
} qk_flow_key;
/* SidekickMulti over a packet batch (sidekick_multi.rs:65-90,101-143): every
 * Insert goes to its AddrKey's quACK (created on first use).  Output: the
 * batch's flows in ascending key order, keys[i] and sketches record i
 * (qk_u32_size(threshold) bytes each, ready for qk_u32_merge into the
 * caller's table).  my_addr = own dst ip:port (6 bytes) or NULL.  A Reset
 * packet (dst ip:port == my_addr) wipes EVERY flow, as the sniff loops do
 * (`senders = HashMap::new()`, sidekick_multi.rs:205,265): the output holds
 * only the inserts after the batch's last reset, stats.discarded counts the
 * inserts before it, stats.last_reset_index is its position, and a caller
 * with stats.resets > 0 must clear its own table before merging the output.
 * cap < flows -> QK_E_CAPACITY with *n_flows set.  keys and sketches may
 * both be host memory (two D2H copies at the end) or both device memory of
 * ctx's GPU (written in place by the finalize kernel: nothing crosses PCIe;
 * the caller synchronises `stream` before reading them); mixed -> QK_E_INVAL. */
int qk_u32_encode_flows_device(qk_ctx *ctx, const uint8_t *d_bufs, size_t n, size_t stride,
                               const qk_pkt_meta *d_meta, const uint8_t my_addr[6], uint32_t threshold,
                               qk_flow_key *keys, uint8_t *sketches, size_t cap, size_t *n_flows,
                               qk_pkt_stats *stats, void *stream);
/* The segmented primitive: ids already grouped by flow (device array,
 * segment g = [offsets[g], offsets[g+1]), host offsets, stream order within a
 * segment) -> nseg sketches (qk_u32_size(threshold) bytes each). */
int qk_u32_encode_segments_device(qk_ctx *ctx, const uint32_t *d_ids, const uint64_t *offsets, size_t nseg,
                                  uint32_t threshold, uint8_t *sketches, void *stream);
/* Per-flow quACK snapshots: the quACK the proxy sends after every packet that
 * brings its flow's count to a multiple of frequency_pkts
 * (sidekick_multi.rs:271-283: `let quack = sc.insert(addr_key, id); if
 * quack.count() % frequency_pkts == 0 { bincode::serialize(&quack) .. }`), for
 * a batch grouped by flow: every crossing inside the batch, not only the flow's
 * end-of-batch state.  A segmented prefix encode.
 * d_base: nseg qk_u32 records of qk_u32_size(threshold) bytes in device memory,
 * row g the quACK of flow g before the batch (a flow the table has not seen: a
 * qk_u32_init row).  d_ids and host offsets[nseg + 1]: the batch's ids grouped
 * by flow in arrival order, as in qk_u32_encode_segments_device; a segment
 * holds fewer than 2^32 ids.  d_arrival (may be NULL): a parallel u32 array,
 * the index each packet had in the ungrouped batch, only carried through to
 * d_snap_arrival_out so that a caller can put the snapshots of all flows into
 * the order the reference would have sent them; both NULL or both set.
 * For segment g with base count c0 and local positions j = 0 .. n_g - 1: after
 * packet j the count is c = (c0 + j + 1) mod 2^32, and packet j triggers a
 * snapshot iff c % frequency_pkts == 0, on the wrapped u32 as the reference's
 * u32 does, so a count that wraps to 0 triggers (on purpose not the 64-bit rule
 * of qk_u32_flows_merge_device's due_out).  The snapshot record: threshold,
 * count = c, has_last = 1, last_value = ids[offsets[g] + j] (unreduced),
 * power_sums[k-1] = base.S_k + sum over i <= j of (id_i mod p)^k, canonical.
 * Snapshots come out ordered by flow, then by position: snap_offsets[nseg + 1]
 * (host) is their CSR index by flow, d_snap_seg_out[r] = g, d_snap_pos_out[r] =
 * offsets[g] + j, d_snap_arrival_out[r] = d_arrival[offsets[g] + j].
 * d_final_out (may be NULL): nseg records, the end-of-batch state of every
 * flow, qk_u32_merge(base_g, the encode of segment g); base_g unchanged for an
 * empty segment: the caller's table update needs no second pass over the ids.
 * NULL ctx -> QK_E_INVAL before any other check; threshold 0 or > 1024 ->
 * QK_E_THRESHOLD; frequency_pkts == 0, decreasing offsets, nseg >= 2^32, a
 * segment of 2^32 ids or more, a host pointer where a device one is required or
 * the reverse, one arrival pointer without the other, an output range
 * overlapping an input or another output (d_final_out against d_base included)
 * -> QK_E_INVAL; a base record whose threshold field differs (found on the
 * device) -> QK_E_MISMATCH, the outputs unspecified; cap < the snapshots ->
 * QK_E_CAPACITY with *n_snap and snap_offsets fully written and no device
 * output written (a repeat with a larger cap gives the same result); nseg == 0
 * -> QK_OK with snap_offsets[0] = 0.  Synchronous on `stream`; every array is
 * 4-byte aligned. */
int qk_u32_snapshot_segments_device(qk_ctx *ctx, const uint8_t *d_base, const uint32_t *d_ids,
                                    const uint32_t *d_arrival, const uint64_t *offsets, size_t nseg,
                                    uint32_t threshold, uint32_t frequency_pkts, uint8_t *d_snap_out,
                                    uint32_t *d_snap_seg_out, uint64_t *d_snap_pos_out,
                                    uint32_t *d_snap_arrival_out, size_t cap, uint64_t *snap_offsets,
                                    size_t *n_snap, uint8_t *d_final_out, void *stream);
/* The proxy's frequency loop on captured packets
 * (sidekick_multi.rs:240-287, start_sidekick_multi_frequency_pkts), against a
 * flow table held by AddrKey in device memory: qk_u32_encode_flows_device's
 * packet front joined with qk_u32_snapshot_segments_device's every-crossing
 * walk.  For records i = 0 .. n - 1 in order, classified exactly as
 * qk_u32_encode_flows_device classifies them (skip on direction, protocol or
 * not-UDP; then Reset if key[6..12] == my_addr; then skip on a length !=
 * QK_BUFFER_SIZE; else Insert of (key, id)):
 *   Reset   the table becomes empty, every flow goes (:263-266);
 *   Insert  the flow's quACK (the table's, or a fresh qk_u32_init(threshold))
 *           takes the id; when its new count is a multiple of frequency_pkts,
 *           on the wrapping u32 as in qk_u32_snapshot_segments_device (a count
 *           that wraps to 0 emits), packet i emits a snapshot (:271-283).
 * Table in: d_keys[n_table] strictly ascending in memcmp order with d_sk record
 * j (qk_u32_size(threshold) bytes) the quACK of key j: a flow array as
 * qk_u32_flows_merge_device keeps it.  Outputs:
 *   the snapshots in ascending i, the reference's send order: d_snap_out row r
 *   the qk_u32 record of the flow right after its packet (last_value the raw
 *   id), d_snap_key_out[r] its key, d_snap_index_out[r] = i.  Snapshots emitted
 *   in front of a Reset inside the batch are part of the output; their sums
 *   build on the table of their epoch: the input table in front of the first
 *   Reset, an empty one behind each Reset;
 *   the table after the last packet, d_keys_out / d_sk_out (*n_table_out rows,
 *   keys strictly ascending): the input table united with the batch when the
 *   batch holds no Reset (a row the batch touched replaced by its end-of-batch
 *   record, the others copied), else only the flows inserted behind the last
 *   Reset;
 *   stats as qk_u32_encode_flows_device gives them (discarded: the Inserts in
 *   front of the last Reset; they did emit).  With frequency_pkts == 1,
 *   *n_snap == inserted + discarded.
 * All d_* arguments are device memory of ctx's GPU, 4-byte aligned (d_bufs:
 * any alignment); my_addr (NULL: no packet resets), n_table_out, n_snap and
 * stats are host memory.  NULL ctx -> QK_E_INVAL before any other check;
 * threshold 0 or > 1024 -> QK_E_THRESHOLD; frequency_pkts == 0, a stride
 * outside 67 .. 512, n >= 2^32, n_table >= 2^31, a host pointer where a device
 * one is required or the reverse, a misaligned array, an output range
 * overlapping an input or another output, input keys not strictly ascending
 * (found on the device) -> QK_E_INVAL; a table record of another threshold ->
 * QK_E_MISMATCH; table_cap or snap_cap too small -> QK_E_CAPACITY with
 * *n_table_out, *n_snap and stats set and no output array written (a repeat
 * with larger caps gives the same result; a call whose caps are both at least
 * the batch's Inserts never needs one); n == 0 -> QK_OK, the table copied, no
 * snapshots.  A batch with Resets runs the chain once per epoch between them
 * (Resets are rare: one per receiver request, media_client.rs:272).
 * Synchronous on `stream`. */
int qk_u32_snapshot_flows_device(qk_ctx *ctx, const uint8_t *d_bufs, size_t n, size_t stride,
                                 const qk_pkt_meta *d_meta, const uint8_t my_addr[6], uint32_t threshold,
                                 uint32_t frequency_pkts, const qk_flow_key *d_keys, const uint8_t *d_sk,
                                 size_t n_table, qk_flow_key *d_keys_out, uint8_t *d_sk_out, size_t table_cap,
                                 size_t *n_table_out, uint8_t *d_snap_out, qk_flow_key *d_snap_key_out,
                                 uint32_t *d_snap_index_out, size_t snap_cap, size_t *n_snap, qk_pkt_stats *stats,
                                 void *stream);

/* ------------------------------------------------------------------------
 * Decode-missing root test.  Replaces media_client.rs:306-313:
 *   for id in log { if arithmetic::eval(&coeffs, id).value() == 0 { hit } }
 * Hit positions (indices into the log) are returned ascending (log order);
 * every log entry congruent to a root is a hit, duplicates included.
 * With stop_at_value != 0 only positions before the first entry equal to
 * stop_value are returned (the `break` at media_client.rs:307-309).
 * *n_hits is set to the number of hits; cap < *n_hits -> QK_E_CAPACITY.
 * ---------------------------------------------------------------------- */
int qk_u32_root_test_device(qk_ctx *ctx, const uint32_t *coeffs, uint32_t d, const uint32_t *d_log,
                            size_t n, int stop_at_value, uint32_t stop_value, uint64_t *hits,
                            size_t cap, size_t *n_hits, void *stream);
int qk_u64_root_test_device(qk_ctx *ctx, const uint64_t *coeffs, uint32_t d, const uint64_t *d_log,
                            size_t n, int stop_at_value, uint64_t stop_value, uint64_t *hits,
                            size_t cap, size_t *n_hits, void *stream);
/* Shard form of the root test for a log cut into contiguous shards across
 * ranks: as above on this shard, and *stop_index is set to the
 * position of the first entry equal to stop_value in the shard, or n when
 * there is none (or stop_at_value == 0).  The global result is the union of
 * shard hits (offset by shard base) below the smallest shard_base+stop_index;
 * sidekick_amd/dist.py: root_test_sharded does that merge with two small
 * collectives. */
int qk_u32_root_test_shard_device(qk_ctx *ctx, const uint32_t *coeffs, uint32_t d, const uint32_t *d_log,
                                  size_t n, int stop_at_value, uint32_t stop_value, uint64_t *hits,
                                  size_t cap, size_t *n_hits, uint64_t *stop_index, void *stream);
int qk_u64_root_test_shard_device(qk_ctx *ctx, const uint64_t *coeffs, uint32_t d, const uint64_t *d_log,
                                  size_t n, int stop_at_value, uint64_t stop_value, uint64_t *hits,
                                  size_t cap, size_t *n_hits, uint64_t *stop_index, void *stream);
/* The distinct roots in GF(p), ascending, of the monic polynomial
 * z^d + c_1 z^(d-1) + ... + c_d (coeffs as qk_*_to_coeffs writes them; any
 * value is taken mod p).  An entry x of a log is a root-test hit
 * (media_client.rs:310, eval(&coeffs, x) == 0) exactly when x mod p is one of
 * them: the device root test scans the log against this set (O(1) per entry)
 * when that beats d Horner steps per entry.  gcd(P, z^(p-1) - 1) and
 * Cantor-Zassenhaus splitting on the host, O(d^2 log p).  *k = number of
 * roots (<= d); cap < *k -> QK_E_CAPACITY. */
int qk_u32_roots(const uint32_t *coeffs, uint32_t d, uint32_t *roots, uint32_t cap, uint32_t *k);
int qk_u64_roots(const uint64_t *coeffs, uint32_t d, uint64_t *roots, uint32_t cap, uint32_t *k);
/* decode_with_log on the device: to_coeffs(diff) on the host (O(t^2)), then
 * the root test over the device-resident log.  diff->count == 0 -> no hits;
 * diff->count > threshold -> QK_E_UNDECODABLE. */
int qk_u32_decode_device(qk_ctx *ctx, const qk_u32 *diff, const uint32_t *d_log, size_t n,
                         int stop_at_last, uint64_t *hits, size_t cap, size_t *n_hits, void *stream);
int qk_u64_decode_device(qk_ctx *ctx, const qk_u64 *diff, const uint64_t *d_log, size_t n,
                         int stop_at_last, uint64_t *hits, size_t cap, size_t *n_hits, void *stream);

/* ------------------------------------------------------------------------
 * Batched per-flow decode: the decode twin of the segmented encode.  A sender
 * that serves many flows holds one diff quACK per flow (one per AddrKey, what
 * SidekickMulti emits: sidekick_multi.rs:65-90) and runs media_client.rs:296-313
 * for each; these two calls do it for nseg flows in one pass.
 * `diffs` holds nseg consecutive qk_u32 records of qk_u32_size(threshold)
 * bytes, exactly what qk_u32_encode_flows_device / _segments_device write,
 * in host memory or in device memory of ctx's GPU.  A record whose threshold
 * field differs from `threshold` -> QK_E_MISMATCH for the whole call.  All
 * outputs are host memory; both calls are synchronous on `stream`.
 * ---------------------------------------------------------------------- */
/* diff_quack.to_coeffs() (the :304 step of media_client.rs:296-313) for nseg diff
 * sketches of one threshold (one per flow, sidekick_multi.rs:65-90), Newton's identities on
 * the device.  coeffs is [nseg][threshold]: row g holds c_1..c_d in its first
 * degrees[g] entries, bit-equal to qk_u32_to_coeffs on record g, zero after
 * them.  status[g] is QK_OK, or QK_E_UNDECODABLE when count > threshold (then
 * degrees[g] == 0; the call itself still returns QK_OK). */
int qk_u32_to_coeffs_segments_device(qk_ctx *ctx, const uint8_t *diffs, size_t nseg, uint32_t threshold,
                                     uint32_t *coeffs, uint32_t *degrees, int32_t *status, void *stream);
/* Log entries per work item of the batched root test: a longer segment is cut
 * into slices of this many entries, one workgroup each. */
#define QK_SEG_DECODE_ITEM 2048u
/* Whole shorter segments are packed into one work item: a run ends after at most this many segments, */
#define QK_SEG_DECODE_MAXSEG 256u
/* and after at most QK_SEG_DECODE_COEF_WORDS / threshold (>= 1) of them: the words of their rows. */
#define QK_SEG_DECODE_COEF_WORDS 8192u
/* decode_with_log (media_client.rs:296-313) for nseg (diff, log segment)
 * pairs in one pass — the per-flow quACKs of sidekick_multi.rs:65-90 against
 * the sender's logs kept grouped by flow: d_log is a device array, segment g
 * = [offsets[g], offsets[g+1]) with host offsets (nseg + 1, non-decreasing),
 * as in qk_u32_encode_segments_device.  hits receives positions into d_log,
 * ascending (segment order, then log order); hit_offsets[nseg + 1] is their
 * CSR index by segment.  Segment g's slice minus offsets[g] is what
 * qk_u32_decode_host(diff_g, log + offsets[g], ...) returns: count == 0 -> no
 * hits, every entry congruent to a root is a hit (duplicates included), and
 * with stop_at_last the segment is cut at its own first entry equal to
 * diff_g->last_value (when has_last).  status[g]: QK_OK, or QK_E_UNDECODABLE
 * (count > threshold: no hits for g; the call still returns QK_OK).
 * *n_hits = total hits; cap < total -> QK_E_CAPACITY with hit_offsets fully
 * written.  nseg == 0 -> QK_OK with hit_offsets[0] = 0. */
int qk_u32_decode_segments_device(qk_ctx *ctx, const uint8_t *diffs, const uint32_t *d_log,
                                  const uint64_t *offsets, size_t nseg, uint32_t threshold, int stop_at_last,
                                  uint64_t *hits, size_t cap, uint64_t *hit_offsets, int32_t *status,
                                  size_t *n_hits, void *stream);

/* ------------------------------------------------------------------------
 * Batched sender step: listen_for_quacks_power_sum (media_client.rs:223-323)
 * for nseg flows whose sent logs stay in device memory.  Per flow g with a
 * quACK (sidekick_amd/receiver.py QuackReceiver.on_quack is the same loop; the
 * reset debounce stays with the caller):
 *   peer.last_value == mine.last_value, compared as an Option (:233) -> IDLE:
 *     mine_out = mine, drain 0, no hits.
 *   idx = first position of segment g whose raw id equals peer.last_value
 *     (:240-246; none when the peer has no last value).
 *   mine1 = mine with log[off_g .. off_g + idx] inserted (:247-252): power sums
 *     of id mod p added, count += idx + 1 (wrapping), last_value = that entry.
 *   reset bits from mine1.count, peer.count and threshold in u32 arithmetic
 *     (:257-261); any set -> action = their OR, mine_out = mine1 (the reference
 *     inserts the prefix before it tests, and keeps it when the reset is
 *     debounced), drain 0, no hits.
 *   otherwise action = ADVANCED, drain = idx + 1, diff = mine1 - peer as
 *     qk_u32_sub_assign (:295-296); the hits are what qk_u32_decode_host(diff,
 *     segment, stop_at_last = 1) returns (:304-313; none when diff.count == 0),
 *     and mine_out = mine1 with qk_u32_remove(id) once per hit (:318-322).
 * A flow without a quACK (d_present[g] == 0) behaves like IDLE.
 * ---------------------------------------------------------------------- */
#define QK_SND_IDLE            0u  /* no quACK for the flow, or last_value unchanged (media_client.rs:233) */
#define QK_SND_ADVANCED        1u  /* prefix inserted, decoded, drain[g] entries to drop (:295-322)       */
#define QK_SND_RESET_REORDERED 2u  /* reset0: quack.last_value not in the log (:258)                      */
#define QK_SND_RESET_RETX      4u  /* reset1: my count < quack count (:259)                               */
#define QK_SND_RESET_EXCEEDS   8u  /* reset2: my count > quack count + threshold, u32 wrap (:260)         */
/* d_mine, d_peer, d_mine_out: nseg qk_u32 records of qk_u32_size(threshold)
 * bytes in device memory of ctx's GPU, row g for flow g; d_present: nseg
 * device bytes or NULL (every flow has a quACK); d_log and host
 * offsets[nseg + 1] as in qk_u32_decode_segments_device.  action, drain, hits,
 * hit_offsets and n_hits are host memory; hits / hit_offsets as in
 * qk_u32_decode_segments_device (global positions into d_log, ascending, CSR
 * by segment).  Synchronous on `stream`.
 * NULL ctx -> QK_E_INVAL before any other check; threshold 0 or > 1024 ->
 * QK_E_THRESHOLD; a host pointer where a device one is required (or the
 * reverse), decreasing offsets, or d_mine_out overlapping an input ->
 * QK_E_INVAL; a record whose threshold field differs -> QK_E_MISMATCH;
 * cap < total -> QK_E_CAPACITY with *n_hits and every output but hits written
 * (a repeat with a larger cap gives the same outputs); nseg == 0 -> QK_OK with
 * hit_offsets[0] = 0. */
int qk_u32_sender_step_segments_device(qk_ctx *ctx, const uint8_t *d_mine, const uint8_t *d_peer,
                                       const uint8_t *d_present, const uint32_t *d_log, const uint64_t *offsets,
                                       size_t nseg, uint32_t threshold, uint8_t *d_mine_out, uint8_t *action,
                                       uint64_t *drain, uint64_t *hits, size_t cap, uint64_t *hit_offsets,
                                       size_t *n_hits, void *stream);
/* seqno_ids.drain(..idx + 1) (media_client.rs:298,316) for all flows: segment
 * g of the output is segment g of the input without its first drain[g]
 * entries; offsets_out[nseg + 1] (host) is its CSR index, offsets_out[0] = 0.
 * d_aux / d_aux_out: an optional parallel u32 array (the seqnos) moved alike,
 * both NULL or both set.  drain[g] > the segment's length -> QK_E_INVAL;
 * cap < the entries remaining -> QK_E_CAPACITY with offsets_out written; an
 * output overlapping an input -> QK_E_INVAL.  Synchronous on `stream`. */
int qk_u32_log_drain_segments_device(qk_ctx *ctx, const uint32_t *d_log, const uint32_t *d_aux,
                                     const uint64_t *offsets, const uint64_t *drain, size_t nseg,
                                     uint32_t *d_log_out, uint32_t *d_aux_out, size_t cap, uint64_t *offsets_out,
                                     void *stream);
/* seqno_ids.push((seqno, id)) (media_client.rs:110 for every packet sent,
 * :318-322 for every retransmission) for a batch of n_new sent packets over
 * nseg flows, with the drain of :298,316 in the same pass: segment g of the
 * output is segment g of the input without its first drain[g] entries (drain
 * == NULL: nothing is drained), followed by every new entry i with
 * d_new_flow[i] == g in ascending i.  The batch arrives ungrouped, in send
 * order; the placement is stable, so a flow's log stays in send order.
 * d_aux / d_new_aux / d_aux_out: the optional parallel u32 array (the seqnos)
 * moved alike; aux mode is d_aux_out != NULL, in which d_aux is required when
 * the input holds any entry and d_new_aux when n_new > 0; outside it both must
 * be NULL.  n_new == 0 (d_new_* may be NULL) is exactly the drain.  offsets,
 * drain and offsets_out[nseg + 1] (offsets_out[0] = 0) are host memory, every
 * d_* device memory of ctx's GPU, 4-byte aligned; cap counts entries of
 * d_log_out (and d_aux_out).  The flow set is the caller's: a new flow is an
 * empty segment, a flow without traffic keeps its place.  Synchronous on
 * `stream`.
 * NULL ctx -> QK_E_INVAL before any other check; nseg == 0 -> QK_OK with
 * offsets_out[0] = 0 (QK_E_INVAL when n_new > 0); decreasing offsets, drain[g]
 * > the segment's length, n_new or nseg >= 2^32, a host pointer where a device
 * one is required or the reverse, an output range overlapping an input range
 * or the other output -> QK_E_INVAL; a d_new_flow[i] >= nseg (found on the
 * device) -> QK_E_INVAL before any output array is written, offsets_out then
 * unspecified; cap < the entries of the result -> QK_E_CAPACITY with
 * offsets_out fully written and no output array written (a repeat with a
 * larger cap gives the same result). */
int qk_u32_log_update_segments_device(qk_ctx *ctx, const uint32_t *d_log, const uint32_t *d_aux,
                                      const uint64_t *offsets, const uint64_t *drain, size_t nseg,
                                      const uint32_t *d_new_flow, const uint32_t *d_new_ids,
                                      const uint32_t *d_new_aux, size_t n_new, uint32_t *d_log_out,
                                      uint32_t *d_aux_out, size_t cap, uint64_t *offsets_out, void *stream);

/* ------------------------------------------------------------------------
 * Device-resident flow table: SidekickMulti's `senders: HashMap<AddrKey,
 * PowerSumQuackU32>` (sidekick_multi.rs:36,65-90) kept in HBM as a "flow
 * array": n qk_flow_key plus n qk_u32 records of qk_u32_size(threshold) bytes,
 * keys strictly ascending in memcmp order of their 12 bytes — exactly what
 * qk_u32_encode_flows_device writes.  The three calls are stateless: the
 * caller owns every table buffer, the context supplies scratch only.  Every
 * flow array is device memory of ctx's GPU, 4-byte aligned, n < 2^31.  All
 * three are synchronous on `stream`.  A host pointer where a device pointer is
 * required, a misaligned array, or an output range that overlaps an input
 * range -> QK_E_INVAL.  Input keys that are not strictly ascending (an
 * adjacent pair out of order or equal, in a or in b; found on the device
 * during the join) -> QK_E_INVAL; a record whose threshold field differs from
 * `threshold` -> QK_E_MISMATCH; after either the outputs are unspecified.
 * Sizes of 0 are valid (merge copies, diff copies a, lookup finds nothing).
 * ---------------------------------------------------------------------- */
#define QK_FLOW_JOIN_TILE 2048u   /* keys of a and b together per work item of the join */

/* table ∪ batch: the per-flow `senders.entry(key).or_insert(new).insert(id)`
 * of sidekick_multi.rs:65-90 for a whole encoded batch.
 * Key in both: qk_u32_merge(a_rec, b_rec), b the later stream.
 * Key in one only: that record, copied.
 * Output ascending.
 * due_out (device, cap bytes, may be NULL): due_out[r] = 1 iff output r has a b source and
 *   (before + b.count) / frequency_pkts > before / frequency_pkts, evaluated in 64 bits,
 *   where before = the a source's count, or 0 without one.
 *   This flags the flows for which start_sidekick_multi_frequency_pkts
 *   (sidekick_multi.rs:274) would have emitted during the batch; the quACKs
 *   themselves, one per crossing, come from qk_u32_snapshot_segments_device.
 *   0 otherwise, and all 0 when frequency_pkts == 0.
 * *n_out = flows in the union.
 * cap < *n_out -> QK_E_CAPACITY with *n_out set and no output array written. */
int qk_u32_flows_merge_device(qk_ctx *ctx, const qk_flow_key *d_keys_a, const uint8_t *d_sk_a, size_t na,
                              const qk_flow_key *d_keys_b, const uint8_t *d_sk_b, size_t nb, uint32_t threshold,
                              uint32_t frequency_pkts, qk_flow_key *d_keys_out, uint8_t *d_sk_out,
                              uint8_t *d_due_out, size_t cap, size_t *n_out, void *stream);

/* media_client.rs:295-296 for every flow of a (mine) against b (the peer's quACKs).
 * d_diffs_out[i] = a[i], and where a's key i is in b, qk_u32_sub_assign by that b record
 *   (sums subtract mod p, count wraps, last_value stays a's).
 * na records in a's key order: what qk_u32_decode_segments_device takes.
 * b keys absent from a are ignored.
 * *n_matched = keys present in both. */
int qk_u32_flows_diff_device(qk_ctx *ctx, const qk_flow_key *d_keys_a, const uint8_t *d_sk_a, size_t na,
                             const qk_flow_key *d_keys_b, const uint8_t *d_sk_b, size_t nb, uint32_t threshold,
                             uint8_t *d_diffs_out, size_t *n_matched, void *stream);

/* SidekickMulti::quack(&addr_key) (sidekick_multi.rs:92-94) for nk keys.
 * keys, sketches and found are HOST memory.
 * keys may come in any order, repeats allowed.
 * found[i] = 1 and sketches record i = the flow's record when the key is in the table.
 * Otherwise found[i] = 0 and record i = qk_u32_init(threshold). */
int qk_u32_flows_lookup_device(qk_ctx *ctx, const qk_flow_key *d_keys, const uint8_t *d_sk, size_t n,
                               uint32_t threshold, const qk_flow_key *keys, size_t nk, uint8_t *sketches,
                               uint8_t *found, void *stream);

/* ------------------------------------------------------------------------
 * Device wire leg: the message between the proxy's flow table and the sender's
 * step, built and parsed where the records live.  The image is the one of
 * qk_u32_serialize / qk_u32_deserialize: u64 threshold, threshold u32 power
 * sums, the u8 Option tag of last_value, last_value (u32, only when the tag
 * is 1), u32 count; little-endian, nothing aligned; 4 * threshold + 13 or + 17
 * bytes.  Both calls are synchronous on `stream`.
 * NULL ctx -> QK_E_INVAL before any other check; threshold 0 or > 1024 ->
 * QK_E_THRESHOLD; a host pointer where a device one is required or the
 * reverse, n (or nseg) >= 2^32, an output range overlapping an input range or
 * another output -> QK_E_INVAL.  Records, keys, rows, lengths and flow indices
 * are 4-byte aligned; the image buffers may have any byte alignment.
 * ---------------------------------------------------------------------- */
/* the longest image of a threshold: 4 * threshold + 17 */
size_t qk_u32_wire_max(uint32_t threshold);

/* status of a well-formed image that a later one for the same flow replaced */
#define QK_WIRE_SUPERSEDED 1

/* bincode::serialize(&quack) per due flow (sidekick_multi.rs:274-283) for the
 * selected flows of a flow array (d_keys, d_sk: n records of
 * qk_u32_size(threshold) bytes).  d_select: n device bytes, non-zero = emit
 * the flow (what qk_u32_flows_merge_device writes as due_out); NULL = every
 * flow.  The m selected flows come out in array order: image r at d_wire_out +
 * r * stride, byte-equal to qk_u32_serialize of the record (4 bytes shorter
 * when has_last == 0), its length in d_len_out[r], its key in d_keys_out[r]
 * (may be NULL; d_keys may then be NULL too), its row index in the input in
 * d_rows_out[r] (may be NULL).  stride >= qk_u32_wire_max(threshold) and
 * < 2^32, odd values included, else QK_E_INVAL.  Bytes of a slot past its length are
 * unspecified; nothing is written outside the m * stride bytes of the slots.
 * *n_out = m; cap < m -> QK_E_CAPACITY with *n_out set and no output array
 * written.  A selected record whose threshold field differs from `threshold`
 * (found on the device) -> QK_E_MISMATCH, the outputs unspecified. */
int qk_u32_flows_emit_device(qk_ctx *ctx, const qk_flow_key *d_keys, const uint8_t *d_sk, size_t n,
                             uint32_t threshold, const uint8_t *d_select, size_t stride,
                             qk_flow_key *d_keys_out, uint32_t *d_rows_out, uint8_t *d_wire_out,
                             uint32_t *d_len_out, size_t cap, size_t *n_out, void *stream);

/* bincode::deserialize(&buf[..len]) per datagram (media_client.rs:226-227) for
 * a batch of n received datagrams, placed by flow: datagram i lies at d_wire +
 * i * stride, d_len[i] bytes long, and belongs to flow d_flow[i] (the caller
 * knows it from the socket; the reference sends no key).  status[i] (host, n
 * entries) is what qk_u32_deserialize returns for those bytes into a sketch of
 * `threshold`: QK_OK, QK_E_FORMAT, or QK_E_MISMATCH for a well-formed image of
 * another threshold; d_len[i] > stride -> QK_E_FORMAT.  No byte past
 * min(d_len[i], stride) of a slot is read, whatever the image claims.
 * Last wins — a rule of the batch (the reference handles one datagram per loop
 * turn; quACKs are cumulative, so a sender that received several for a flow
 * since its last step needs only the newest as long as the losses of all of
 * them together stay <= threshold; beyond that the newest alone ends in
 * QK_SND_RESET_EXCEEDS where stepping each would have recovered every packet:
 * qk_u32_wire_ingest_queue_device keeps them all): among the accepted datagrams of
 * flow g the one with the largest i goes to row g of d_peer (nseg records of
 * qk_u32_size(threshold) bytes; the threshold field set to `threshold`) with
 * d_present[g] = 1, and the flow's earlier accepted datagrams get status
 * QK_WIRE_SUPERSEDED (a caller that wants every quACK stepped takes
 * qk_u32_wire_ingest_queue_device and qk_u32_sender_steps_segments_device).  A flow without an accepted datagram gets d_present[g] = 0
 * and keeps its d_peer row.  *n_accepted = the winners.
 * A d_flow[i] >= nseg (found on the device) -> QK_E_INVAL before d_peer or
 * d_present is written.  n == 0 -> QK_OK with d_present all zero; nseg == 0
 * with n > 0, or stride == 0 -> QK_E_INVAL. */
int qk_u32_wire_ingest_device(qk_ctx *ctx, const uint8_t *d_wire, size_t stride, const uint32_t *d_len,
                              const uint32_t *d_flow, size_t n, uint32_t threshold, size_t nseg,
                              uint8_t *d_peer, uint8_t *d_present, int32_t *status, size_t *n_accepted,
                              void *stream);

/* ------------------------------------------------------------------------
 * Every queued quACK of a flow stepped in one call: the loop of
 * media_client.rs:223-323 over ALL datagrams a batch brought for a flow, one
 * per loop turn as the reference takes them, where qk_u32_wire_ingest_device
 * and qk_u32_sender_step_segments_device take the newest only.
 * ---------------------------------------------------------------------- */
/* qk_u32_wire_ingest_device's inputs, validation (one rule set) and status[i]
 * values, but nothing is superseded: every accepted image is parsed into a
 * qk_u32 record of d_queue (cap records of qk_u32_size(threshold) bytes, the
 * threshold field set to `threshold`), the records grouped by flow and, within
 * a flow, in arrival order (ascending i; the placement is stable).
 * q_offsets[nseg + 1] (host, q_offsets[0] = 0) is their CSR index by flow,
 * *n_accepted = q_offsets[nseg].  cap < *n_accepted -> QK_E_CAPACITY with
 * q_offsets, status and *n_accepted written and d_queue untouched.  A
 * d_flow[i] >= nseg (found on the device) -> QK_E_INVAL before any output
 * array is written; nseg == 0 with n > 0, stride == 0, n >= 2^32, nseg >=
 * 2^32 - 1 (the sort key of a rejected datagram is nseg), d_queue overlapping
 * an input, a host pointer where a device one is required or the reverse ->
 * QK_E_INVAL.  n == 0 -> QK_OK, q_offsets all
 * zero.  Synchronous on `stream`. */
int qk_u32_wire_ingest_queue_device(qk_ctx *ctx, const uint8_t *d_wire, size_t stride, const uint32_t *d_len,
                                    const uint32_t *d_flow, size_t n, uint32_t threshold, size_t nseg,
                                    uint8_t *d_queue, size_t cap, uint64_t *q_offsets, int32_t *status,
                                    size_t *n_accepted, void *stream);

/* action of a queued quACK behind its flow's first reset: not stepped */
#define QK_SND_UNSTEPPED 16u
/* Per flow g, with step() = what qk_u32_sender_step_segments_device does for
 * one flow and one quACK:
 *   m = mine[g]; b = 0
 *   for j in 0 .. k_g - 1, q = q_offsets[g] + j:       the flow's quACKs in queue order
 *     (m, action, d, missing) = step(m, queue[q], log_g[b ..], threshold)
 *     q_action[q] = action; q_drain[q] = d; hits of q = missing + b (+ offsets[g])
 *     a reset bit in action: stop; the later quACKs of the flow keep
 *       QK_SND_UNSTEPPED, q_drain 0 and no hits
 *     b += d
 *   mine_out[g] = m; drain[g] = b; stepped[g] = the quACKs consumed (the
 *   resetting one included).
 * The log is not moved: b is an offset, the drain stays with
 * qk_u32_log_update_segments_device.  The intervals of successive quACKs are
 * disjoint and ascending, so hits (global positions into d_log) ascend over
 * the whole call; hit_offsets[nq + 1] is their CSR index by quACK, nq =
 * q_offsets[nseg].  A flow stops at its first reset because the debounce is
 * the caller's and depends on time: when the reset fires, the flow is cleared
 * and its later quACKs change nothing; when it is held back, the caller goes
 * on from mine_out with a second call on the unstepped tail.  A flow with k_g
 * == 0 is idle; with k_g <= 1 everywhere the outputs equal
 * qk_u32_sender_step_segments_device's.
 * d_mine, d_mine_out: nseg records; d_queue: nq records, q_offsets[nseg + 1]
 * (host, q_offsets[0] = 0) as qk_u32_wire_ingest_queue_device writes them;
 * d_log / offsets as in the single step.  q_action, q_drain (nq entries),
 * stepped, drain (nseg), hits, hit_offsets and n_hits are host memory.
 * Synchronous on `stream`.
 * NULL ctx -> QK_E_INVAL before any other check; threshold 0 or > 1024 ->
 * QK_E_THRESHOLD; a host pointer where a device one is required (or the
 * reverse), decreasing offsets or q_offsets, q_offsets[0] != 0, or d_mine_out
 * overlapping an input -> QK_E_INVAL; a record of mine or of the queue whose
 * threshold field differs -> QK_E_MISMATCH; cap < total -> QK_E_CAPACITY with
 * *n_hits and every output but hits written (a repeat with a larger cap gives
 * the same outputs); nseg == 0 -> QK_OK with hit_offsets[0] = 0. */
int qk_u32_sender_steps_segments_device(qk_ctx *ctx, const uint8_t *d_mine, const uint8_t *d_queue,
                                        const uint64_t *q_offsets, const uint32_t *d_log, const uint64_t *offsets,
                                        size_t nseg, uint32_t threshold, uint8_t *d_mine_out, uint8_t *q_action,
                                        uint64_t *q_drain, uint32_t *stepped, uint64_t *drain, uint64_t *hits,
                                        size_t cap, uint64_t *hit_offsets, size_t *n_hits, void *stream);

/* ------------------------------------------------------------------------
 * Multi-GPU: the id stream cut into contiguous shards, one
 * per GPU in global rank order, merged with ONE RCCL reduce over xGMI.
 * The reference callers are single processes (sidekick.rs:58-127,
 * sender.rs:80-116), so a communicator can drive several GPUs from one
 * process; one process per GPU works the same way.
 *   - one process, several GPUs:  qk_comm_create(ndev, devices)
 *     (ncclCommInitAll; local rank i = global rank i = devices[i]);
 *   - one process per GPU:        rank 0 calls qk_comm_unique_id and ships
 *     the QK_COMM_ID_BYTES bytes to the other ranks by any channel, then
 *     every rank calls qk_comm_init_rank(id, rank, world, device);
 *   - collectives over a host channel: qk_comm_init_host (below).
 * Each local rank owns its own qk_ctx.  Array arguments (d_ids, n, d_log,
 * streams) have one entry per LOCAL rank (qk_comm_info's nlocal), in local
 * rank order.  streams may be NULL (every local rank uses its device's null
 * stream); the work runs on the context's stream, ordered after the given
 * stream, and the given stream is ordered after it.  Every rank of the
 * communicator must make the same sequence of collective calls with the same
 * threshold and root.
 * Failure semantics: a rank whose own arguments or local work fail — including
 * the staging copy of its payload into a collective — still takes part in
 * every collective of the call (its failure travels as data), so no peer is
 * left blocked; see each call for what every rank returns.  A failed
 * collective, or a rank that cannot read what a collective delivered, aborts
 * the communicator (ncclCommAbort): that call and every later one return
 * QK_E_COMM; destroy it.  An abort releases this process's ranks only; a peer
 * in another process is released by its own timeout: every wait on an RCCL
 * collective polls ncclCommGetAsyncError and aborts after the communicator's
 * timeout (qk_comm_set_timeout; a host channel's callbacks time out
 * themselves), and the rank's own work in front of the collective is waited
 * for under 4 x that timeout, also polling the asynchronous error.
 * ---------------------------------------------------------------------- */
typedef struct qk_comm qk_comm;
#define QK_COMM_ID_BYTES 128
int qk_comm_unique_id(uint8_t id[QK_COMM_ID_BYTES]);
int qk_comm_create(int ndev, const int *devices, qk_comm **out);
int qk_comm_init_rank(const uint8_t id[QK_COMM_ID_BYTES], int rank, int world, int device, qk_comm **out);
/* One rank on `device` whose collectives run through the caller's host
 * channel instead of RCCL: the identical sharded protocol, every collective
 * staged through pinned host memory (the async encode completes before it
 * returns).  For more ranks than GPUs (RCCL takes one rank per device) and for
 * ranks RCCL cannot connect.  Each callback acts as the collective of its name
 * over all ranks (uint64 elements, wrapping sums; allgather: recv[r*n .. r*n+n)
 * = rank r's send) and returns 0, nonzero on failure (-> QK_E_COMM). */
typedef struct qk_comm_host_ops {
    void *user;
    int (*reduce_sum_u64)(void *user, uint64_t *buf, size_t n, int root);
    int (*broadcast_u64)(void *user, uint64_t *buf, size_t n, int root);
    int (*allgather_u64)(void *user, const uint64_t *send, uint64_t *recv, size_t n);
} qk_comm_host_ops;
int qk_comm_init_host(const qk_comm_host_ops *ops, int rank, int world, int device, qk_comm **out);
void qk_comm_destroy(qk_comm *comm);
/* world size, local ranks in this process, global rank of local rank 0 */
int qk_comm_info(const qk_comm *comm, int *world, int *nlocal, int *first_rank);
/* the qk_ctx of a local rank (owned by the communicator, valid until
 * qk_comm_destroy: profiling, grid knobs, and the single-GPU calls on that
 * device) */
int qk_comm_context(qk_comm *comm, int local, qk_ctx **out);
/* all ranks reach this point (one 8-byte reduce), then the local streams drain */
int qk_comm_barrier(qk_comm *comm);
/* Waits on RCCL collectives give up after `ms` milliseconds (0: never;
 * default 300 000), abort the communicator and return QK_E_COMM — the bound
 * on how long a rank waits for a peer that failed in another process. */
int qk_comm_set_timeout(qk_comm *comm, int64_t ms);
/* What RCCL itself reports for local rank `local`: ncclCommCount (ranks),
 * ncclCommCuDevice (device), ncclCommUserRank (rank) — e.g. to check that a
 * multi-process launch joined one communicator of the expected size.
 * QK_E_INVAL for a host-channel communicator (no RCCL communicator). */
int qk_comm_rccl_info(const qk_comm *comm, int local, int *count, int *device, int *rank);

/* Sharded encode: local rank i encodes d_ids[i][0 .. n[i]) on its GPU, then
 * one ncclReduce(sum, uint64) of its partial to global rank `root`:
 * (t + 1) power-sum/count words (u64 ids: 2t + 1, 32-bit limbs), a
 * (has_last, last) slot per rank, so the root learns the last id of the last
 * non-empty shard without a second collective, and a failed-rank count.  The
 * root merges the whole stream into q (as if inserted after q's content);
 * other ranks leave q untouched.  _async only enqueues; _wait (every rank)
 * drains the local streams and merges on the root.
 * Failures: a rank whose shard argument is bad (non-device, misaligned) or
 * whose encode fails returns that error from _async and _wait and sends a
 * failed payload; the root then returns QK_E_PEER (or its own error) and
 * leaves q untouched. */
int qk_u32_encode_sharded_async(qk_comm *comm, const uint32_t *const *d_ids, const size_t *n, uint32_t threshold,
                                int root, void *const *streams);
int qk_u64_encode_sharded_async(qk_comm *comm, const uint64_t *const *d_ids, const size_t *n, uint32_t threshold,
                                int root, void *const *streams);
int qk_u32_encode_sharded_wait(qk_comm *comm, qk_u32 *q);
int qk_u64_encode_sharded_wait(qk_comm *comm, qk_u64 *q);
int qk_u32_encode_sharded(qk_comm *comm, const uint32_t *const *d_ids, const size_t *n, qk_u32 *q, int root,
                          void *const *streams);
int qk_u64_encode_sharded(qk_comm *comm, const uint64_t *const *d_ids, const size_t *n, qk_u64 *q, int root,
                          void *const *streams);
/* Sharded decode over a candidate log cut the same way (log shard i on local
 * rank i): the root turns diff into coefficients (diff is read on the root
 * only; other ranks may pass NULL) and broadcasts them, every rank
 * root-tests its shard, the shards' stop positions, hit counts and statuses
 * are all-gathered, then the hits.  Every rank returns the single-GPU
 * qk_*_decode_device result for the whole log (global positions, ascending,
 * cut at the first entry equal to diff->last_value when stop_at_last).  Any
 * failure — an undecodable diff on the root, a bad log shard or a failed root
 * test on any rank — makes every rank return the same status (the lowest
 * failing rank's). */
int qk_u32_decode_sharded(qk_comm *comm, const qk_u32 *diff, int root, const uint32_t *const *d_log, const size_t *n,
                          int stop_at_last, uint64_t *hits, size_t cap, size_t *n_hits, void *const *streams);
int qk_u64_decode_sharded(qk_comm *comm, const qk_u64 *diff, int root, const uint64_t *const *d_log, const size_t *n,
                          int stop_at_last, uint64_t *hits, size_t cap, size_t *n_hits, void *const *streams);

/* ------------------------------------------------------------------------
 * Synthetic identifier streams (benchmarks/tests): counter-based splitmix64,
 * id_i = mix(seed + (start+i+1)*0x9E3779B97F4A7C15); u32 ids = high 32 bits.
 * ---------------------------------------------------------------------- */
int qk_fill_splitmix_u32(qk_ctx *ctx, uint32_t *d_out, size_t n, uint64_t seed, uint64_t start,
                         void *stream);
int qk_fill_splitmix_u64(qk_ctx *ctx, uint64_t *d_out, size_t n, uint64_t seed, uint64_t start,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QUACK_HIP_H */
