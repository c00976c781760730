/*
 * aipstack_amd -- MI355X (gfx950) Internet-checksum engine: the C-ABI boundary.
 *
 * Plain C, plain pointers and sizes: callable from C, C++, cgo, ctypes, JNI.
 * Implemented by libaipstack_chksum.so (aipstack_amd/lib/), which holds the host
 * C++ code and the hand-written CDNA4 HIP kernels.
 *
 * Two kinds of entry point:
 *
 * 1. The per-packet link-time hook of the reference,
 *      uint16_t IpChksumInverted(char const *data, size_t len);
 *    which replaces the inline default in reference src/aipstack/infra/Chksum.h:77-99
 *    when the consumer compiles with -DAIPSTACK_EXTERNAL_CHKSUM (declaration at
 *    Chksum.h:50-51; contract at Chksum.h:54-76). This one runs on the HOST: a GPU
 *    launch (microseconds) costs more than the whole scalar computation of one packet.
 *
 * 2. The batch entry points (aipstack_chksum_batch_*): the reference has no batch API
 *    (every caller -- IpChksum(ptr,len) Chksum.h:122-125, IpChksumAccumulator::addIpBuf
 *    Chksum.h:283-315 -- processes one packet at a time), so these are new. Each is the
 *    batched equivalent of a reference call, evaluated for many packets at once on the
 *    GPU. All pointers named d_* are DEVICE pointers (hipMalloc'd or HIP-registered);
 *    the work is enqueued on `stream` (a hipStream_t; NULL = the legacy default stream)
 *    and is complete when the stream is. Nothing here allocates or synchronises.
 *    There is no CPU fallback: on a host without a usable gfx950 device these return
 *    AIPSTACK_CHKSUM_EHIP / _ENODEV.
 *
 * Results are bit-exact with the reference for every packet whose length satisfies
 * the reference precondition len <= 65535 (Chksum.h:73-74).
 */
#ifndef AIPSTACK_AMD_CHKSUM_H
#define AIPSTACK_AMD_CHKSUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (0 = success, negative = failure) ---------------------------- */
#define AIPSTACK_CHKSUM_OK      0
#define AIPSTACK_CHKSUM_EINVAL (-1) /* bad argument: null pointer, len > 65535, n too big */
#define AIPSTACK_CHKSUM_EHIP   (-2) /* HIP runtime error (see aipstack_chksum_last_hip_error) */
#define AIPSTACK_CHKSUM_ENODEV (-3) /* no gfx950 device visible to this process */

/* Largest packet length the reference admits (Chksum.h:73-74). */
#define AIPSTACK_CHKSUM_MAX_LEN 65535u

/* Largest slot stride of the frame batches on ring slots (their 64-frame header window must
 * span at most 4 MiB); a larger one is _EINVAL. */
#define AIPSTACK_CHKSUM_MAX_SLOT_STRIDE 65536u

/* ---- flags for the batch entry points ------------------------------------------ */
/* Write IpChksum (= ~IpChksumInverted, Chksum.h:122-125) instead of the inverted sum. */
#define AIPSTACK_CHKSUM_FINAL 1u
/* Hint (results are identical with or without it): the batch's bytes were written by device
 * kernels with ordinary (write-back) stores since they were last read -- e.g. segments
 * assembled on the device just before their checksum. On gfx950 a cached read of such a line
 * costs the memory side far more than a streaming one, so the batch is then read without
 * touching any of its lines through the L2-allocating path (config A: 242-258 us against
 * 285-312 for the default form; the default form is faster on bytes that arrived by DMA or
 * streaming stores, and on bytes read before). Honoured by aipstack_chksum_batch_strided
 * (back-to-back packets of >= 1 KiB: boundary segments captured from the stream; packets at a
 * stride: their edge segments read nontemporal), aipstack_chksum_batch_slotted (edge segments
 * nontemporal) and the chain batches (payload pieces that lie back to back read as column runs
 * with their boundary segments captured from the stream, CHAIN 322.5 against 365.3 us on
 * plain-written chains; other layouts: edge segments nontemporal); ignored elsewhere. */
#define AIPSTACK_CHKSUM_JUST_WRITTEN 4u

/* ---- 1. per-packet host hook ----------------------------------------------------- */

/* Replaces reference Chksum.h:77-99 (declared at Chksum.h:51 under
 * AIPSTACK_EXTERNAL_CHKSUM). Inverted checksum (ones'-complement sum of big-endian
 * 16-bit words; odd tail byte padded with a zero low byte) of `len` bytes at `data`,
 * any alignment. data must not be null; len <= 65535. Pure, reentrant, thread-safe. */
uint16_t IpChksumInverted(const char *data, size_t len);

/* ---- 2. batch entry points (device-resident, stream-ordered) -------------------- */

/* Fixed-stride batch: packet i is the `len` bytes at d_base + i*stride, for i < n.
 * d_out[i] = IpChksumInverted(packet i)   (or IpChksum(...) with AIPSTACK_CHKSUM_FINAL).
 * Batched equivalent of n calls of reference IpChksumInverted (Chksum.h:77-99) /
 * IpChksum (Chksum.h:122-125). d_base may have any byte alignment. */
int aipstack_chksum_batch_strided(const void *d_base, uint64_t stride, uint32_t len,
                                  uint64_t n, uint16_t *d_out, uint32_t flags,
                                  void *stream);

/* CSR batch: packet i is bytes [d_offsets[i], d_offsets[i+1]) of d_base (n+1 offsets,
 * non-decreasing, each packet <= 65535 bytes; starts may be odd).
 * d_out[i] as for the strided form. */
int aipstack_chksum_batch_csr(const void *d_base, const uint64_t *d_offsets,
                              uint64_t n, uint16_t *d_out, uint32_t flags,
                              void *stream);

/* Ring-slot batch: packet i is the d_len[i] bytes at d_base + i*slot_stride -- a receive
 * ring that holds one frame per fixed-size slot with its length beside it (the TAP driver
 * reads one frame per buffer, reference tap/linux/TapDeviceLinux.cpp:156-178), checksummed
 * where it lies, without compacting it first. The buffer holds n whole slots; each
 * d_len[i] <= min(slot_stride, 65535) (a longer one is clamped to that and reported through
 * aipstack_chksum_contract_violations). d_out[i] as for the strided form. */
int aipstack_chksum_batch_slotted(const void *d_base, uint64_t slot_stride, const uint32_t *d_len,
                                  uint64_t n, uint16_t *d_out, uint32_t flags, void *stream);

/* Seeded CSR batch: d_out[i] = IpChksumAccumulator(State{d_states[i]})
 *                                  .getChksum(IpBufRef{packet i})
 * i.e. a per-packet saved accumulator state (pseudo-header / header words, exported by
 * IpChksumAccumulator::getState, Chksum.h:171-184) resumed and completed over the
 * packet bytes (Chksum.h:263-269, 283-315). Writes the FINAL checksum (as getChksum
 * does). A state of 0 with no header words is the plain IpChksum(IpBufRef). */
int aipstack_chksum_batch_seeded_csr(const void *d_base, const uint64_t *d_offsets,
                                     const uint32_t *d_states, uint64_t n,
                                     uint16_t *d_out, void *stream);

/* Chained (scatter-gather) batch: chain i is the chunks [d_chunk_index[i],
 * d_chunk_index[i+1]) of the chunk table, taken in order as one logical byte sequence:
 * chunk k is the d_chunk_len[k] bytes at DEVICE address d_chunk_addr[k] (any alignment,
 * each <= 65535 bytes). This is an IpBufRef chain (reference Buf.h:68-251) flattened into
 * the non-empty chunks ipBufProcessBytes visits (BufUtils.h:129-178). With
 * AIPSTACK_CHKSUM_FINAL, d_out[i] = IpChksumAccumulator(State{s_i}).getChksum(chain i)
 * (Chksum.h:171-174, 263-315), s_i = d_states[i] or 0 when d_states is NULL; without
 * the flag, the bitwise NOT of that (the inverted sum). n+1 index entries. */
int aipstack_chksum_batch_chain(const uint64_t *d_chunk_addr, const uint32_t *d_chunk_len,
                                const uint64_t *d_chunk_index, const uint32_t *d_states,
                                uint64_t n, uint16_t *d_out, uint32_t flags, void *stream);

/* Flag of aipstack_chksum_batch_chain_fill: a computed checksum of 0 is sent as 0xFFFF
 * (UDP, reference udp/IpUdpProto.h:176-178). */
#define AIPSTACK_CHKSUM_ZERO_AS_FFFF 2u

/* The send side of the chained batch: the reference's Tx call sites sum a pseudo-header
 * State, the header node and the payload chunks, then write the checksum into the header
 * (tcp/IpTcpProto_output.h:1251-1277, udp/IpUdpProto.h:164-179, ip/IpStack.h:1184).
 * Computes the FINAL checksum of chain i into d_out[i] as aipstack_chksum_batch_chain does,
 * then (a second, stream-ordered pass) stores it big-endian at DEVICE address
 * d_field_addr[i] (any alignment; 0 = no store). As in the reference, the field's two bytes
 * must read 0 when the batch runs (they are summed), and no field may lie inside another
 * chain's bytes. Flags: AIPSTACK_CHKSUM_ZERO_AS_FFFF. */
int aipstack_chksum_batch_chain_fill(const uint64_t *d_chunk_addr, const uint32_t *d_chunk_len,
                                     const uint64_t *d_chunk_index, const uint32_t *d_states,
                                     const uint64_t *d_field_addr, uint64_t n,
                                     uint16_t *d_out, uint32_t flags, void *stream);

/* ---- frame-level batches: Rx verify / Tx fill on raw Ethernet frames ------------------ */

/* Per-frame verdicts of aipstack_chksum_rx_verify (and statuses of _tx_fill), restating the
 * reference's receive-path decisions that involve checksums or the lengths they cover:
 * eth/EthIpIface.h:367-390, ip/IpStack.h:936-1018 and :1093-1130 (ICMP),
 * tcp/IpTcpProto_input.h:68-100, udp/IpUdpProto.h:470-490 and :631-652. Checks that need
 * stack state (interface addresses, listeners, reassembly) stay with the host. */
#define AIPSTACK_RX_NOT_IP4            0 /* < 14 bytes or EtherType != 0x0800 (e.g. ARP) */
#define AIPSTACK_RX_DROP_IP_MALFORMED  1 /* IPv4 header/length checks fail (IpStack.h:938-990) */
#define AIPSTACK_RX_DROP_IP_CHKSUM     2 /* IPv4 header checksum bad (IpStack.h:1016) */
#define AIPSTACK_RX_FRAGMENT           3 /* header OK, MF or offset set: host reassembles */
#define AIPSTACK_RX_DROP_L4_MALFORMED  4 /* TCP < 20 B, UDP length bad, ICMP < 8 B */
#define AIPSTACK_RX_DROP_L4_CHKSUM     5 /* TCP/UDP/ICMP checksum bad */
#define AIPSTACK_RX_ACCEPT             6 /* every checksum present verified */
#define AIPSTACK_RX_ACCEPT_NO_CHKSUM   7 /* UDP with checksum field 0 = none (IpUdpProto.h:637) */
#define AIPSTACK_RX_ACCEPT_OTHER       8 /* IPv4 header OK; protocol other than TCP/UDP/ICMP */

/* Rx verify: frame i = bytes [d_offsets[i], d_offsets[i+1]) of d_base (an Ethernet frame,
 * as the TAP driver delivers it); d_verdict[i] = one of AIPSTACK_RX_*. Read-only.
 * Frame offsets (here and in the Tx fills) are non-decreasing (n+1 entries) and each frame
 * is at most 65535 bytes, so that 64 consecutive frames span at most 4 MiB: the kernels
 * read a 64-frame chunk's header bytes through one range-checked window over that span.
 * Offsets outside this contract give unspecified verdicts (never accesses outside the
 * chunk's span). */
int aipstack_chksum_rx_verify(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                              uint8_t *d_verdict, void *stream);

/* Tx fill, IN PLACE: for each IPv4 frame, write the IPv4 header checksum (field taken as 0,
 * ip/IpStack.h:425-453) and, unless it is a fragment, the TCP / UDP (0 -> 0xFFFF) / ICMP
 * checksum (tcp/IpTcpProto_output.h:1251-1277, udp/IpUdpProto.h:164-179,
 * ip/IpStack.h:1164-1190). d_status[i]: AIPSTACK_RX_ACCEPT (filled), _ACCEPT_OTHER (IPv4
 * header only), _FRAGMENT (IPv4 header only), _NOT_IP4 / _DROP_*_MALFORMED (untouched,
 * or IPv4 header only for L4-malformed). Frames must not overlap. */
int aipstack_chksum_tx_fill(void *d_base, const uint64_t *d_offsets, uint64_t n,
                            uint8_t *d_status, void *stream);

/* Tx fill in two stream-ordered passes, same results as aipstack_chksum_tx_fill: a read pass
 * computes every frame's fields into d_workspace (8 bytes per frame, 8-byte aligned, at
 * least aipstack_chksum_tx_fill_workspace_bytes(n) bytes, owned by the caller and free
 * again once the stream passes the call), then a scatter pass stores them into the frames.
 * Round 5: no faster than the one pass at any batch size measured (1 M frames: 194.5 vs
 * 193.4 us); for callers that want the stores as a pass of their own. */
uint64_t aipstack_chksum_tx_fill_workspace_bytes(uint64_t n);
int aipstack_chksum_tx_fill_split(void *d_base, const uint64_t *d_offsets, uint64_t n,
                                  uint8_t *d_status, void *d_workspace,
                                  uint64_t workspace_bytes, void *stream);

/* The split fill's read pass alone: per frame the 8-byte record the scatter pass would
 * apply, frames untouched -- for a caller that applies the fields itself (the host-memory
 * engine's Tx fill, or a NIC path that patches headers on the way out). Record of frame i:
 * bits 0-15 the IPv4 header checksum, 16-31 the L4 checksum (the field values, big-endian
 * when stored), 32-39 the L4 field's offset from the frame start, bit 40 = write the IPv4
 * field (at offset 24), bit 41 = write the L4 field, bits 48-55 the status (AIPSTACK_RX_*).
 * d_records 8-byte aligned, n entries. */
int aipstack_chksum_tx_fill_records(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                                    uint64_t *d_records, void *stream);

/* The frame batches on a ring of slots (layout as aipstack_chksum_batch_slotted: frame i is
 * the d_len[i] bytes at d_base + i*slot_stride, 0 < slot_stride <=
 * AIPSTACK_CHKSUM_MAX_SLOT_STRIDE, else _EINVAL; n whole slots): Rx verify, the one-pass
 * in-place Tx fill, the split fill (records pass + scatter pass through a caller-owned
 * workspace, as aipstack_chksum_tx_fill_split), and the Tx records. Same results per frame as
 * the CSR forms. */
int aipstack_chksum_rx_verify_slotted(const void *d_base, uint64_t slot_stride,
                                      const uint32_t *d_len, uint64_t n, uint8_t *d_verdict,
                                      void *stream);
int aipstack_chksum_tx_fill_slotted(void *d_base, uint64_t slot_stride, const uint32_t *d_len,
                                    uint64_t n, uint8_t *d_status, void *stream);
int aipstack_chksum_tx_fill_slotted_split(void *d_base, uint64_t slot_stride,
                                          const uint32_t *d_len, uint64_t n, uint8_t *d_status,
                                          void *d_workspace, uint64_t workspace_bytes,
                                          void *stream);
int aipstack_chksum_tx_fill_records_slotted(const void *d_base, uint64_t slot_stride,
                                            const uint32_t *d_len, uint64_t n,
                                            uint64_t *d_records, void *stream);

/* ---- header-split Tx fill: a header ring + send-ring chunks -------------------------- */

/* Status of aipstack_chksum_tx_fill_hsplit: the segment's split does not satisfy the layout
 * rule below; nothing of it was written. The caller linearises such a segment
 * (aipstack_tx_linearise) and uses aipstack_chksum_tx_fill. */
#define AIPSTACK_TX_SPLIT_LAYOUT 9
/* Largest d_hdr_len of the header-split fill. */
#define AIPSTACK_CHKSUM_MAX_SPLIT_HEADER 256u

/* Tx fill of segments as the reference's send side builds them: a header node in its own
 * buffer followed by chunks of the send ring (tcp/IpTcpProto_output.h:1251-1277,
 * udp/IpUdpProto.h:164-179, ip/IpStack.h:632-663), filled where they lie. Segment i is one
 * Ethernet frame in two parts: its first d_hdr_len[i] bytes at d_hdr + i*hdr_stride, the rest
 * the chunks [d_chunk_index[i], d_chunk_index[i+1]) of the chunk table, in order (form and
 * contract of aipstack_chksum_batch_chain: any alignment, each chunk <= 65535 bytes, n+1 index
 * entries; 0 chunks = e.g. a pure ACK). With L = d_hdr_len[i] + its chunk bytes, the result is
 * what aipstack_chksum_tx_fill does to the L-byte linearised frame: the same d_status[i], the
 * same IPv4 header checksum and TCP / UDP (0 -> 0xFFFF) / ICMP checksum stored big-endian into
 * the header slot (fragments, other protocols and L4-malformed segments: the IPv4 field only;
 * _NOT_IP4 and _DROP_IP_MALFORMED: untouched). Both fields are taken as 0 whatever they hold,
 * so a call can be repeated (or replayed from a graph). Payload chunks are never written.
 *
 * Layout rule (else d_status[i] = AIPSTACK_TX_SPLIT_LAYOUT, segment untouched):
 * d_hdr_len[i] <= min(hdr_stride, AIPSTACK_CHKSUM_MAX_SPLIT_HEADER); every byte the linear
 * fill would parse or write lies in the header slot, stage by stage -- the Ethernet header
 * (14 bytes), the 20-byte IPv4 minimum, the IPv4 header with options (14 + 4*IHL), the fixed
 * L4 header (TCP 20, UDP 8, ICMP 8): a frame that has a stage's bytes (by L) while
 * d_hdr_len[i] does not cover them is out of layout; and for a non-fragment TCP / UDP / ICMP
 * segment the bytes the L4 checksum covers (total length - header length, or the UDP length)
 * end exactly at L (no trailing padding).
 *
 * Three stream-ordered passes: a header pass (parse, IPv4 checksum, the L4 sum's seed), the
 * chained batch over the chunk table, a finish pass that stores the fields and d_status.
 * d_workspace: caller-owned, 8-byte aligned, at least
 * aipstack_chksum_tx_fill_hsplit_workspace_bytes(n) (<= 16*n + 256) bytes, free again once the
 * stream passes the call. flags: AIPSTACK_CHKSUM_JUST_WRITTEN (the payload read); other bits
 * are ignored. _EINVAL before any work for a null pointer, hdr_stride == 0, n > 2^40, a short
 * or misaligned workspace; n == 0 is a no-op. Oversized chunks: _CHUNK_LEN (diagnostics). */
uint64_t aipstack_chksum_tx_fill_hsplit_workspace_bytes(uint64_t n);
int aipstack_chksum_tx_fill_hsplit(void *d_hdr, uint64_t hdr_stride, const uint32_t *d_hdr_len,
                                   const uint64_t *d_chunk_addr, const uint32_t *d_chunk_len,
                                   const uint64_t *d_chunk_index, uint64_t n,
                                   uint8_t *d_status, void *d_workspace,
                                   uint64_t workspace_bytes, uint32_t flags, void *stream);

/* ---- linearise: header-split segments into the linear frames of a send ring ------------ */

/* Per-segment outcomes of aipstack_tx_linearise / aipstack_tx_linearise_slotted. A segment
 * with several faults takes the earliest in this order: skipped, invalid, too short, too
 * large, wrong room. */
#define AIPSTACK_TX_LIN_WRITTEN    17 /* the L bytes of the frame are in place */
#define AIPSTACK_TX_LIN_SKIPPED    18 /* the producer emitted nothing for this segment */
#define AIPSTACK_TX_LIN_INVALID    19 /* header length, a chunk length or the index breaks the contract */
#define AIPSTACK_TX_LIN_TOO_SHORT  20 /* L < 14: sendFrame's HardwareError */
#define AIPSTACK_TX_LIN_TOO_LARGE  21 /* L > frame_max: sendFrame's PacketTooLarge */
#define AIPSTACK_TX_LIN_WRONG_ROOM 22 /* offsets form: L is not d_offsets[i+1] - d_offsets[i] */

/* The batched form of the copy in the reference's driver: TapDeviceLinux::sendFrame
 * (tap/linux/TapDeviceLinux.cpp:109-140) rejects a frame shorter than the Ethernet header
 * (HardwareError) or longer than the frame MTU (PacketTooLarge), copies the IpBufRef chain into
 * one linear buffer (ipBufTakeBytes) and write()s it. These calls do the checks and the copy
 * for n segments at once; the write() and its errno handling stay with the host. The result
 * is what the ring-slot and CSR calls of this header take (Rx verify, Tx fill, TCP Rx parse,
 * IPv4 reassembly, the host-memory engine), and what a caller linearises a segment of status
 * AIPSTACK_TX_SPLIT_LAYOUT with.
 *
 * Segment i is what aipstack_chksum_tx_fill_hsplit takes, and what aipstack_tcp_tx_segment and
 * aipstack_udp_tx_fragment make: the first d_hdr_len[i] bytes at d_hdr + i*hdr_stride, then the
 * chunks [d_chunk_index[i], d_chunk_index[i+1]) of the chunk table in order (any alignment,
 * each chunk <= 65535 bytes, n+1 index entries, 0 chunks allowed); L = d_hdr_len[i] + its chunk
 * bytes. Frame i goes to d_frames + i*slot_stride (0 < slot_stride <=
 * AIPSTACK_CHKSUM_MAX_SLOT_STRIDE; the ring holds n whole slots) or to d_frames + d_offsets[i]
 * (n+1 offsets; frame i has the room d_offsets[i+1] - d_offsets[i]).
 *
 * d_status[i] (AIPSTACK_TX_LIN_*) and d_frame_len[i] (L where the frame was written, else 0)
 * are stored for all n segments in every call, so outputs depend on inputs only and a call can
 * be replayed from a graph:
 *   skipped     d_hdr_len[i] == 0 (as aipstack_udp_tx_fragment leaves for an invalid datagram),
 *               or d_seg_status (may be NULL) holds AIPSTACK_TX_BURST_INVALID or
 *               AIPSTACK_TX_DGRAM_INVALID for it. Every other value of d_seg_status is
 *               linearised, AIPSTACK_TX_SPLIT_LAYOUT included.
 *   invalid     d_hdr_len[i] > min(hdr_stride, AIPSTACK_CHKSUM_MAX_SPLIT_HEADER); an index that
 *               decreases; a chunk over 65535 bytes (also sets the sticky _CHUNK_LEN violation,
 *               as the chained batch does).
 *   too short   L < 14.
 *   too large   L > frame_max.
 *   wrong room  offsets form: L != d_offsets[i+1] - d_offsets[i].
 * The chunk lengths are summed in table order and the sum stops after the first chunk that
 * brings it above frame_max, so a garbage index costs a bounded walk; a chunk over 65535 bytes
 * behind that point is not looked at (the segment is then too large, not invalid).
 *
 * Bytes: nothing outside [frame start, frame start + L) of a written frame is ever stored -- not
 * a slot's slack, not the slot or room of a skipped or rejected segment, not the bytes between
 * CSR frames. Reads follow the chained batch: only aligned 16-byte segments that hold a byte of
 * a header's first d_hdr_len[i] bytes or of a chunk, so a chunk may end at its allocation's
 * last byte. The destination must not overlap the header ring, any chunk, or the tables; frames
 * must not overlap each other. Frame stores are nontemporal (the next reader is a DMA engine
 * or the Rx kernels). No allocation, no synchronisation, no workspace; two stream-ordered
 * launches (a plan pass, a copy pass), capturable into a graph.
 *
 * flags: AIPSTACK_CHKSUM_JUST_WRITTEN is honoured: the payload chunks are then read with
 * nontemporal loads (header slots always with ordinary ones); results are identical either way.
 * Other bits are ignored. _EINVAL before any work for a null pointer (d_seg_status excepted), a
 * zero stride, frame_max == 0, frame_max > 65535, frame_max > slot_stride, slot_stride >
 * AIPSTACK_CHKSUM_MAX_SLOT_STRIDE, n > 2^40. n == 0 is a no-op that returns _OK before the
 * arguments are looked at (as aipstack_chksum_tx_fill_hsplit), whatever else is passed. */
int aipstack_tx_linearise_slotted(const void *d_hdr, uint64_t hdr_stride, const uint32_t *d_hdr_len,
                                  const uint64_t *d_chunk_addr, const uint32_t *d_chunk_len,
                                  const uint64_t *d_chunk_index, uint64_t n,
                                  const uint8_t *d_seg_status, void *d_frames,
                                  uint64_t slot_stride, uint32_t frame_max, uint32_t *d_frame_len,
                                  uint8_t *d_status, uint32_t flags, void *stream);
int aipstack_tx_linearise(const void *d_hdr, uint64_t hdr_stride, const uint32_t *d_hdr_len,
                          const uint64_t *d_chunk_addr, const uint32_t *d_chunk_len,
                          const uint64_t *d_chunk_index, uint64_t n, const uint8_t *d_seg_status,
                          void *d_frames, const uint64_t *d_offsets, uint32_t frame_max,
                          uint32_t *d_frame_len, uint8_t *d_status, uint32_t flags, void *stream);

/* ---- TCP burst segmentation: headers, chunk table and checksums of a data burst -------- */

/* The reference sends a burst of one connection's data as a loop: pcb_output_active ->
 * pcb_output_segment -> PcbOutputHelper::sendSegment -> IpStack::sendIp4DgramFast
 * (tcp/IpTcpProto_output.h:1056-1120, 1218-1335, ip/IpStack.h:564-663). What is common to the
 * burst is prepared once (prepareCommon, prepareSendIp4Dgram: ports, ack, window, addresses,
 * both partial checksum States); per segment only seq_num, the PSH / FIN bits, tcp_len, the
 * IPv4 total length, ident (m_next_id++) and the two checksums change. This is that loop for a
 * batch of bursts: the host hands over one descriptor per burst, the GPU emits every segment's
 * complete 54-byte frame header, the chunk table of its data and both checksums, in the layout
 * aipstack_chksum_tx_fill_hsplit, aipstack_chksum_batch_chain and a scatter-gather sender take.
 * Deciding what to send (window, retransmission, the TCP state machine) stays with the host. */
#define AIPSTACK_TCP_SEGMENT_HEADER 54u   /* Ethernet 14 + IPv4 20 (IHL 5) + TCP 20 (offset 5) */
#define AIPSTACK_TCP_BURST_FIN 1u         /* burst flag: the last segment carries FIN|PSH */
#define AIPSTACK_TX_BURST_INVALID 10      /* per-segment status: its burst breaks the contract */

typedef struct aipstack_tcp_burst {       /* 96 bytes, 8-byte aligned, host-made */
    uint64_t data_addr[2];  /* DEVICE addresses of the burst's bytes: a range of the circular send
                               buffer is at most two pieces (utils/TcpRingBufferUtils.h:51,113);
                               piece 1 follows piece 0; any alignment */
    uint32_t data_len[2];   /* bytes in each piece; their sum D must fit 32 bits */
    uint32_t seq;           /* sequence number of the burst's first byte (snd_una + offset, :1102) */
    uint32_t psh_offset;    /* snd_psh_index relative to the burst start: PSH on the segment with
                               start < psh_offset <= start + len (:1096-1099); 0 = none */
    uint16_t mss;           /* data bytes per segment: 1 .. 65535 - 40 */
    uint16_t ip_id;         /* Ident of segment 0; segment k gets ip_id + k mod 2^16 (IpStack.h:653) */
    uint8_t  flags;         /* AIPSTACK_TCP_BURST_FIN */
    uint8_t  reserved[3];   /* 0 */
    uint8_t  hdr[56];       /* template, first 54 bytes: the frame header as prepareCommon and
                               prepareSendIp4Dgram leave it */
} aipstack_tcp_burst;

/* Segments of a burst (:1069-1090), D = data_len[0] + data_len[1]: S = ceil(D / mss) when
 * D > 0; S = 1 when D == 0 and FIN is set (a segment without data); else S = 0 (legal, produces
 * nothing). Segment k: start = k*mss, len = min(mss, D - start); sequence number seq + start
 * (mod 2^32); offset_flags = Tcp4EncodeOffset(5) | Ack, Psh by the psh_offset rule, Fin|Psh on
 * the last segment of a FIN burst; IPv4 total length 40 + len; ident ip_id + k; the IPv4 header
 * checksum as sendIp4DgramFast computes it; the TCP checksum as sendSegment does (pseudo-header,
 * the 20 header bytes, the data chain; a computed 0 stays 0x0000, 0 -> 0xFFFF is UDP's rule).
 * Template: the IPv4 total length, ident and header checksum and the TCP seq, offset/flags and
 * checksum are ignored and overwritten; every other byte (MACs, EtherType, version/IHL/DSCP,
 * flags/fragment offset, TTL, protocol, addresses, ports, ack, window, urgent pointer) is
 * copied. Data: the bytes [start, start + len) of the two-piece range -- one chunk, two for the
 * one segment that straddles the piece boundary, none for a FIN-only segment.
 *
 * Burst contract: mss >= 1; 40 + mss <= 65535; D < 2^32; reserved == 0; no flag bit but FIN;
 * template EtherType 0x0800, version/IHL 0x45, protocol 6; seg_index[b+1] - seg_index[b] == S
 * and chunk_base[b+1] - chunk_base[b] == the burst's chunk count. */

/* Host side, no GPU: segment and chunk counts of each burst as running sums (n_bursts + 1
 * entries each, starting at 0); _EINVAL if a burst breaks the contract above (or for a null
 * pointer, n_bursts > 2^40). */
int aipstack_tcp_burst_layout(const aipstack_tcp_burst *h_bursts, uint64_t n_bursts,
                              uint64_t *h_seg_index, uint64_t *h_chunk_base);

uint64_t aipstack_tcp_tx_segment_workspace_bytes(uint64_t n_segments);   /* <= 16*n + 256 */

/* The batch. d_bursts, d_seg_index, d_chunk_base: the descriptors and the two running sums of
 * aipstack_tcp_burst_layout, in DEVICE memory (non-decreasing, from 0 to n_segments / n_chunks).
 * Segment i is the k-th segment of the burst b that holds it (seg_index[b] <= i <
 * seg_index[b+1], k = i - seg_index[b]). The call leaves:
 *   - its 54 header bytes at d_hdr + i*hdr_stride, the slot's bytes [54, min(hdr_stride, 64))
 *     written as 0 (a 64-byte ring is stored in whole lines), bytes past 64 untouched; slots
 *     are written once, whole, and never read;
 *   - a compact chunk table in the form and contract of aipstack_chksum_batch_chain (no empty
 *     chunks; d_chunk_index[n_segments] = n_chunks; n_chunks entries of d_chunk_addr /
 *     d_chunk_len, n_segments + 1 of d_chunk_index). Within a burst, segment k's first chunk
 *     is chunk_base[b] + k, plus 1 if k lies after the straddling segment;
 *   - d_status[i] = AIPSTACK_RX_ACCEPT.
 * The bytes are what the reference loop produces, and what aipstack_chksum_tx_fill_hsplit
 * leaves when run on the same headers with both fields zeroed.
 * A burst that breaks the contract: every segment the caller's index gives it gets
 * AIPSTACK_TX_BURST_INVALID, its slots stay untouched, and its chunk entries are written with
 * length 0 at address 0 (harmless to the chained batch). Whatever the descriptors hold, only
 * the n_segments slots, the n_chunks entries, the index, d_status and the workspace are
 * written.
 *
 * Three stream-ordered passes through the caller's workspace (8-byte aligned, at least
 * aipstack_tcp_tx_segment_workspace_bytes(n_segments) bytes, free again once the stream passes
 * the call): a plan pass (owner search, validation, chunk table, the L4 seed and the IPv4
 * checksum as arithmetic on header words), the chained batch over the table just written, an
 * emit pass that builds and stores the slots. Never allocates or synchronises; can be captured
 * into a graph and repeated (outputs depend on inputs only). flags:
 * AIPSTACK_CHKSUM_JUST_WRITTEN (the payload read); other bits are ignored. _EINVAL before any
 * work for a null pointer, hdr_stride < 54, n_bursts / n_segments / n_chunks above 2^40, a
 * short or misaligned workspace; n_segments == 0 is a no-op. */
int aipstack_tcp_tx_segment(const aipstack_tcp_burst *d_bursts, const uint64_t *d_seg_index,
                            const uint64_t *d_chunk_base, uint64_t n_bursts,
                            uint64_t n_segments, uint64_t n_chunks,
                            void *d_hdr, uint64_t hdr_stride,
                            uint64_t *d_chunk_addr, uint32_t *d_chunk_len,
                            uint64_t *d_chunk_index, uint8_t *d_status,
                            void *d_workspace, uint64_t workspace_bytes,
                            uint32_t flags, void *stream);

/* ---- UDP send with IPv4 fragmentation: headers, chunk table and checksums of datagrams --- */

/* The reference sends a UDP datagram through UdpApi::sendUdpIp4Packet -> IpStack::sendIp4Dgram ->
 * send_fragmented (udp/IpUdpProto.h:152-184, ip/IpStack.h:373-464, 467-539): one UDP checksum
 * over the whole datagram, then one IPv4 packet per fragment in which only the total length, the
 * flags / fragment offset and the header checksum change while a range of the datagram's buffer
 * is cut into pieces. This is that loop for a batch of datagrams: the host hands over one
 * descriptor per datagram, the GPU emits every fragment's frame header (one, for a datagram that
 * fits its MTU), the chunk table of its data, the IPv4 header checksums and the UDP checksum, in
 * the layout aipstack_chksum_tx_fill_hsplit, aipstack_chksum_batch_chain and a scatter-gather
 * sender take. Routing, the source-address check (checkSendIp4Allowed), ARP and the decision to
 * send stay with the host; IPv4 options are not covered (ICMP sends: aipstack_icmp_rx_respond). */
#define AIPSTACK_UDP_FIRST_FRAGMENT_HEADER 42u /* Ethernet 14 + IPv4 20 (IHL 5) + UDP 8 */
#define AIPSTACK_UDP_NEXT_FRAGMENT_HEADER  34u /* Ethernet 14 + IPv4 20: fragments after the first */
#define AIPSTACK_UDP_MIN_MTU 256u              /* the reference's MinMTU (ip/IpStack.h:255) */
#define AIPSTACK_TX_FRAG_NEEDED   12 /* per datagram: above the MTU with DF set
                                        (IpErr::FragmentationNeeded, ip/IpStack.h:409-411) */
#define AIPSTACK_TX_DGRAM_INVALID 13 /* per fragment / datagram: the datagram breaks the contract */

typedef struct aipstack_udp_dgram {       /* 80 bytes, 8-byte aligned, host-made */
    uint64_t data_addr[2];  /* DEVICE addresses of the UDP payload: at most two pieces, piece 1
                               follows piece 0; any alignment (as aipstack_tcp_burst) */
    uint32_t data_len[2];   /* bytes in each piece; D = their sum, 8 + D <= 65535 */
    uint16_t mtu;           /* IP MTU of the outgoing interface, >= AIPSTACK_UDP_MIN_MTU */
    uint16_t ip_id;         /* Ident of the datagram: EVERY fragment carries it (m_next_id++ runs
                               once per datagram, ip/IpStack.h:434) */
    uint32_t reserved;      /* 0 */
    uint8_t  hdr[48];       /* template, first 42 bytes: Ethernet 14 + IPv4 20 + UDP 8 as
                               Ip4CommonSendParams and UdpTxInfo would fill them */
} aipstack_udp_dgram;

/* Fragments of a datagram, with P = 8 + D (the IP payload), M = mtu - 20 and F = (M / 8) * 8
 * (Ip4RoundFragLen(20, mtu) - 20, proto/Ip4Proto.h:71-73):
 *   - 20 + P <= mtu: S = 1; total length 20 + P; flags / offset the template's (DF allowed);
 *   - else, DF set in the template: S = 0, nothing is emitted, datagram status
 *     AIPSTACK_TX_FRAG_NEEDED (not an error);
 *   - else S = ceil((P - M) / F) + 1: fragment k < S - 1 carries the F bytes at IP-payload offset
 *     k * F with MF set, the last one the rest (up to M bytes: more than F when M is not a
 *     multiple of 8, ip/IpStack.h:497-501); flags / offset (k < S - 1 ? 0x2000 : 0) | k * F / 8;
 *     total length 20 + the fragment's payload bytes.
 * Every fragment: the datagram's Ident; the IPv4 header checksum over its 20 header bytes
 * (ip/IpStack.h:425-453 and :510-515 give the same value). Fragment 0 carries the UDP header:
 * length P, checksum over the pseudo-header (addresses, 17, P), the UDP header and the whole
 * payload, a computed 0 sent as 0xFFFF (udp/IpUdpProto.h:163-179).
 * Template: copied are the MACs, EtherType, version/IHL/DSCP, the DF bit, TTL, protocol, addresses
 * and ports; ignored and overwritten are the IPv4 total length, Ident, MF and fragment offset, the
 * header checksum, the UDP length and the UDP checksum.
 * Data, in UDP-payload coordinates: fragment 0 owns [0, F - 8) ([0, D) when S = 1), fragment
 * k >= 1 owns [k * F - 8, ...): one chunk, two for the one fragment that straddles the piece
 * boundary, none when D = 0. C = the datagram's chunk count.
 *
 * Datagram contract: mtu >= 256; 8 + D <= 65535; reserved == 0; template EtherType 0x0800,
 * version/IHL 0x45, protocol 17, flags / offset word with no bit but DF; frag_index[d+1] -
 * frag_index[d] == S and chunk_base[d+1] - chunk_base[d] == C. */

/* Host side, no GPU: fragment and chunk counts of each datagram as running sums (n_dgrams + 1
 * entries each, starting at 0) and, if h_status is not NULL, each datagram's status
 * (AIPSTACK_RX_ACCEPT, or AIPSTACK_TX_FRAG_NEEDED with S = C = 0); _EINVAL if a datagram breaks
 * the contract above (or for a null pointer, n_dgrams > 2^40). */
int aipstack_udp_dgram_layout(const aipstack_udp_dgram *h_dgrams, uint64_t n_dgrams,
                              uint64_t *h_frag_index, uint64_t *h_chunk_base, uint8_t *h_status);

/* <= 16 * (n_dgrams + n_frags) + 256 */
uint64_t aipstack_udp_tx_fragment_workspace_bytes(uint64_t n_dgrams, uint64_t n_frags);

/* The batch. d_dgrams, d_frag_index, d_chunk_base: the descriptors and the two running sums of
 * aipstack_udp_dgram_layout, in DEVICE memory (non-decreasing, from 0 to n_frags / n_chunks).
 * Fragment i is the k-th fragment of the datagram d that holds it (frag_index[d] <= i <
 * frag_index[d+1], k = i - frag_index[d]). The call leaves:
 *   - its header at d_hdr + i*hdr_stride: 42 bytes (Ethernet, IPv4, UDP) for k = 0, 34 bytes
 *     (Ethernet, IPv4) for k >= 1, d_hdr_len[i] saying which; the slot's bytes from the header's
 *     end up to min(hdr_stride, 64) written as 0 (a 64-byte ring on a 64-byte boundary is stored
 *     in whole lines), bytes past 64 untouched; slots are written once, whole, and never read;
 *   - a compact chunk table in the form and contract of aipstack_chksum_batch_chain (no empty
 *     chunks; d_chunk_index[n_frags] = n_chunks; n_chunks entries of d_chunk_addr / d_chunk_len,
 *     n_frags + 1 of d_chunk_index). Within a datagram, fragment k's first chunk is
 *     chunk_base[d] + k, plus 1 if k lies after the straddling fragment;
 *   - d_status[i] = AIPSTACK_RX_ACCEPT, and per datagram d_dgram_status[d] = AIPSTACK_RX_ACCEPT
 *     or AIPSTACK_TX_FRAG_NEEDED.
 * The bytes are what the reference's three functions produce, and for a datagram of one fragment
 * what aipstack_chksum_tx_fill_hsplit leaves when run on the same header with both fields zeroed.
 * A datagram that breaks the contract: d_dgram_status[d] = AIPSTACK_TX_DGRAM_INVALID, every
 * fragment the caller's index gives it gets that status and d_hdr_len 0, its slots stay
 * untouched, and its chunk entries are written with length 0 at address 0 (harmless to the
 * chained batch); so is a fragment or a chunk entry that the index gives to no datagram.
 * Whatever the descriptors and the two indices hold, only the n_frags slots, d_hdr_len, the
 * n_chunks entries (every one of them, by the lane of its own number), the index, the two status
 * arrays and the workspace are written, and the payload is read only through table entries
 * written by this call.
 *
 * Three stream-ordered passes through the caller's workspace (8-byte aligned, at least
 * aipstack_udp_tx_fragment_workspace_bytes(n_dgrams, n_frags) bytes, free again once the stream
 * passes the call): a plan pass (owner search, validation, chunk table, per-fragment IPv4
 * checksum, per-datagram UDP seed and chain bounds), the chained batch with ONE CHAIN PER
 * DATAGRAM (a datagram's fragments partition its payload in order, so the chunks
 * [chunk_base[d], chunk_base[d+1]) of the table just written are its chain), an emit pass that
 * builds and stores the slots. Never allocates or synchronises; can be captured into a graph and
 * repeated (outputs depend on inputs only). flags: AIPSTACK_CHKSUM_JUST_WRITTEN (the payload
 * read); other bits are ignored. _EINVAL before any work for a null pointer, hdr_stride < 42,
 * n_dgrams / n_frags / n_chunks above 2^40, a short or misaligned workspace; n_frags == 0 is a
 * no-op. */
int aipstack_udp_tx_fragment(const aipstack_udp_dgram *d_dgrams, const uint64_t *d_frag_index,
                             const uint64_t *d_chunk_base, uint64_t n_dgrams, uint64_t n_frags,
                             uint64_t n_chunks, void *d_hdr, uint64_t hdr_stride,
                             uint32_t *d_hdr_len, uint64_t *d_chunk_addr, uint32_t *d_chunk_len,
                             uint64_t *d_chunk_index, uint8_t *d_status, uint8_t *d_dgram_status,
                             void *d_workspace, uint64_t workspace_bytes, uint32_t flags,
                             void *stream);

/* ---- TCP Rx parse: segment metadata, options and PCB lookup of a batch of frames -------- */

/* What the reference does with a TCP datagram once its checksum is good, up to the call of
 * pcb_input (tcp/IpTcpProto_input.h:81-130): read the six TcpSegMeta fields (:81-90,
 * tcp/TcpMiscUtils.h:40-48), bound the data offset and cut the options from the data
 * (:103-122), parse the MSS and window-scale options (ParseTcpOptions, tcp/TcpOptions.h:63-125)
 * and find the PCB by address tuple (find_pcb, tcp/IpTcpProto.h:806-820, ordered by
 * TcpPcbKeyCompare::CompareKeys, tcp/TcpPcbKey.h:50-86) -- for a batch of frames in device
 * memory. The host's Rx loop becomes "for each record with a PCB: pcb_input(pcb, meta, data)".
 * The TCP state machine stays with the host; listeners, RST replies and the local-address /
 * unicast-source checks (they need interface state) are aipstack_tcp_rx_respond's, below. */
#define AIPSTACK_RX_DROP_TCP_OFFSET 11      /* TCP checksum good, data offset outside
                                               [20, datagram length] (IpTcpProto_input.h:108-116) */
#define AIPSTACK_TCP_NO_PCB 0xFFFFFFFFu
#define AIPSTACK_TCP_OPT_MSS 1u             /* = TcpOptionFlags::Mss      */
#define AIPSTACK_TCP_OPT_WND_SCALE 2u       /* = TcpOptionFlags::WndScale */
#define AIPSTACK_TCP_SEG_VALID 0x80u

typedef struct aipstack_tcp_rx_seg {        /* 32 bytes, host byte order */
    uint32_t remote_addr, local_addr;       /* IPv4 source, destination (Ip4Addr::value()) */
    uint16_t remote_port, local_port;       /* TCP source, destination port */
    uint32_t seq_num, ack_num;
    uint16_t flags;                         /* the raw OffsetFlags word */
    uint16_t window_size;
    uint16_t data_off;                      /* first data byte, from the frame start: 14 + 4*IHL + 4*offset */
    uint16_t data_len;                      /* IPv4 total length - 4*IHL - 4*offset (not the frame's length:
                                               Ethernet padding is not data) */
    uint16_t mss;                           /* valid with _OPT_MSS, else 0 */
    uint8_t  wnd_scale;                     /* valid with _OPT_WND_SCALE, else 0 */
    uint8_t  opts;                          /* _OPT_* | _SEG_VALID */
} aipstack_tcp_rx_seg;

typedef struct aipstack_tcp_pcb_key {       /* 16 bytes */
    uint32_t local_addr, remote_addr;
    uint16_t local_port, remote_port;
    uint32_t cookie;                        /* the caller's PCB handle; != AIPSTACK_TCP_NO_PCB */
} aipstack_tcp_pcb_key;

/* Host side, no GPU: sorts the table in place into the order of CompareKeys (ascending by
 * remote_port, then remote_addr, then local_port, then local_addr), the order the lookup
 * searches. _EINVAL for a null pointer with n > 0, n > 2^40, a duplicate key or a cookie equal
 * to AIPSTACK_TCP_NO_PCB; the array is then left as a permutation of its input. */
int aipstack_tcp_pcb_table_sort(aipstack_tcp_pcb_key *h_keys, uint64_t n);

/* The batch (frames as aipstack_chksum_rx_verify / _rx_verify_slotted take them, under the same
 * offsets, span and slot contracts). Per frame i:
 *   - d_verdict[i]: what Rx verify gives, except that a frame it accepts as TCP
 *     (AIPSTACK_RX_ACCEPT, protocol 6) whose data offset 4*(flags >> 12) is below 20 or above
 *     the datagram length becomes AIPSTACK_RX_DROP_TCP_OFFSET;
 *   - d_segs[i]: for an accepted TCP frame with a valid offset the record above, opts / mss /
 *     wnd_scale exactly what ParseTcpOptions leaves for the 4*offset - 20 option bytes (mss and
 *     wnd_scale 0 where their flag is not set); 32 zero bytes for every other frame;
 *   - d_pcb[i]: for a valid record the cookie of the table entry equal to {local_addr,
 *     remote_addr, local_port, remote_port}, else AIPSTACK_TCP_NO_PCB.
 * d_pcbs: n_pcbs entries in DEVICE memory, sorted by aipstack_tcp_pcb_table_sort, keys unique
 * (n_pcbs == 0: no table, d_pcbs may be NULL). An unsorted table gives unspecified d_pcb values,
 * never an access outside the table. Re-upload the table when a PCB is added or removed.
 * Two stream-ordered passes: the Rx verify launch, unchanged, into d_verdict; then a parse
 * pass, one frame per lane, that reads the verdict and (only of frames accepted as TCP) at
 * most the first 134 header bytes, never past the frame's own length. Never allocates or
 * synchronises; can be captured into a graph and repeated (outputs depend on inputs only).
 * _EINVAL before any work for a null pointer, n or n_pcbs above 2^40, d_segs or d_pcbs not
 * 8-byte aligned, d_pcb not 4-byte aligned, a slot stride outside
 * (0, AIPSTACK_CHKSUM_MAX_SLOT_STRIDE]; n == 0 is a no-op. */
int aipstack_tcp_rx_parse(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                          const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                          uint8_t *d_verdict, aipstack_tcp_rx_seg *d_segs, uint32_t *d_pcb,
                          void *stream);
int aipstack_tcp_rx_parse_slotted(const void *d_base, uint64_t slot_stride, const uint32_t *d_len,
                                  uint64_t n, const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                                  uint8_t *d_verdict, aipstack_tcp_rx_seg *d_segs, uint32_t *d_pcb,
                                  void *stream);

/* ---- IPv4 reassembly on receive: fragments linked into datagrams, checksum verified ------ */

/* What the reference does with a fragment between the IPv4 header checks and recvIp4Dgram
 * (ip/IpStack.h:1020-1043, IpReassembly::reassembleIp4, ip/IpReassembly.h:181-386) -- for the
 * datagrams whose fragments all lie in one batch of frames, without the copy into a reassembly
 * buffer (:343-346): the fragments are grouped by the key of find_reass_entry (:409-412: source,
 * destination, ident, protocol), a group that is one complete datagram is linked in offset order,
 * and the TCP / UDP / ICMP checksum is taken over the linked payload as recvIp4Dgram's handlers
 * would take it over the reassembled one (tcp/IpTcpProto_input.h:92-100, udp/IpUdpProto.h:484-489
 * and :631-652, ip/IpStack.h:1093-1130). The host's Rx loop becomes "for each head: build the
 * IpBufNode list from d_next, call recvIp4Dgram; feed the verdict-3 fragments to IpReassembly".
 * Stateless per batch. The local-address test of ip/IpStack.h:1027, expiry, MaxReassEntrys /
 * MaxReassHoles and anything that spans two batches stay with the host. */
#define AIPSTACK_RX_FRAG_MEMBER      14  /* per frame: fragment of a datagram reassembled in this batch */
#define AIPSTACK_RX_DROP_FRAG        15  /* per frame: fragment reassembleIp4 ignores or rejects by itself */
#define AIPSTACK_RX_REASS_TRUNCATED  16  /* per datagram: complete, UDP length < reassembled length: host verifies */
#define AIPSTACK_REASS_NONE 0xFFFFFFFFu

typedef struct aipstack_ip4_dgram {   /* 16 bytes, host byte order; all zero except at a head frame */
    uint32_t n_frags;                 /* >= 2 */
    uint32_t last_frame;              /* frame index of the fragment without MF */
    uint16_t data_len;                /* reassembled IP payload length */
    uint8_t  proto;
    uint8_t  verdict;                 /* AIPSTACK_RX_ACCEPT / _ACCEPT_NO_CHKSUM / _ACCEPT_OTHER /
                                         _DROP_L4_MALFORMED / _DROP_L4_CHKSUM / _REASS_TRUNCATED */
    uint32_t reserved;                /* 0 */
} aipstack_ip4_dgram;

/* The batch (frames as aipstack_chksum_rx_verify / _rx_verify_slotted take them, under the same
 * offsets, span and slot contracts). max_reass_size = the reference's MaxReassSize, 1 .. 65531
 * (ip/IpReassembly.h:96).
 * A FRAGMENT is a frame Rx verify gives AIPSTACK_RX_FRAGMENT: its IP payload is the total length
 * - 4*IHL bytes at frame byte 14 + 4*IHL (options allowed), its offset 8 * (flags_offset &
 * 0x1FFF), its MF bit flags_offset & 0x2000 (ip/IpStack.h:1021-1034). A fragment with an empty
 * payload belongs to no group (reassembleIp4 returns before touching any state, :189-191):
 * verdict AIPSTACK_RX_DROP_FRAG. The other fragments with one key form a GROUP. A group is
 * COMPLETE iff, ordered by offset, its first member has offset 0, each member's offset is the
 * previous one's offset plus its length, MF is set on every member but the last and clear on the
 * last, and no member breaks offset <= max_reass_size && length <= max_reass_size - offset
 * (:219-223). (So: at least two members, no duplicate, no overlap, every length but the last a
 * multiple of 8.) Arrival order is irrelevant; groups may interleave with each other and with
 * other traffic. A group is reassembled entirely or left entirely alone:
 *   - complete: every member gets verdict AIPSTACK_RX_FRAG_MEMBER, d_head[i] = the frame index of
 *     the offset-0 member, d_next[i] = the frame index of the member with the next offset
 *     (AIPSTACK_REASS_NONE on the last), and d_dgram[head] is filled;
 *   - incomplete (a missing piece, a duplicate, an overlap, an extra fragment, two datagrams under
 *     one key, an oversize member): members that break the size bound get AIPSTACK_RX_DROP_FRAG,
 *     every other member keeps AIPSTACK_RX_FRAGMENT with AIPSTACK_REASS_NONE links; the host hands
 *     those to its own IpReassembly in batch order.
 * Every frame that is no member of a complete group has d_head = d_next = AIPSTACK_REASS_NONE and
 * every frame that is no head a d_dgram of 16 zero bytes. d_chunk_addr[i] / d_chunk_len[i]: the
 * payload's device address and length of every fragment with verdict 3 or 14, 0 / 0 for every
 * other frame (and for a verdict-3 frame whose lengths do not bear the verdict out, which only a
 * verdict byte changed under the call can give: it stays 3, in no group, nothing of it read); with d_next this is the datagram's IpBufNode list.
 * Datagram verdict, over data_len = the last member's offset + length: TCP: below 20 bytes
 * _DROP_L4_MALFORMED, else the checksum with the pseudo-header; UDP: UDP length below 8 or above
 * data_len _DROP_L4_MALFORMED, else checksum field 0 _ACCEPT_NO_CHKSUM (the host applies the UDP
 * length, as for a whole frame), else UDP length below data_len AIPSTACK_RX_REASS_TRUNCATED (the
 * reference truncates the chain there, udp/IpUdpProto.h:492; left to the host), else the checksum;
 * ICMP: the checksum; any other protocol _ACCEPT_OTHER.
 *
 * Stream-ordered passes through the caller's workspace (8-byte aligned, at least
 * aipstack_ip4_reass_workspace_bytes(n) bytes -- two open-addressing tables of a power of two of
 * at least 4 entries per frame, cleared by the call, plus 30 bytes per frame -- free again once
 * the stream passes the call): Rx verify, unchanged; a classify pass (it clears the tables; one
 * frame per lane: of a fragment at most the 34 first header bytes, never past the frame's own
 * length whatever the verdict byte says); an insert pass (atomicCAS / atomicOr / atomicAdd on the tables); the chained
 * batch, unchanged, with one one-chunk chain per frame; a link pass (each member's successor); a
 * finish pass (one offset-0 member per lane walks its links, at most min(members of its key, 8192)
 * steps). No lock, no lane waits for another, every probe is bounded by the table size. Never
 * allocates or synchronises; can be captured into a graph and repeated (outputs depend on inputs
 * only, never on which lane won a race). _EINVAL before any work for a null pointer, n > 2^32 - 2,
 * max_reass_size outside 1 .. 65531, d_chunk_addr or the workspace not 8-byte aligned,
 * d_chunk_len / d_next / d_head / d_dgram not 4-byte aligned, a short workspace, a slot stride
 * outside (0, AIPSTACK_CHKSUM_MAX_SLOT_STRIDE]; n == 0 is then a no-op. */
uint64_t aipstack_ip4_reass_workspace_bytes(uint64_t n);
int aipstack_ip4_rx_reassemble(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                               uint32_t max_reass_size, uint8_t *d_verdict, uint64_t *d_chunk_addr,
                               uint32_t *d_chunk_len, uint32_t *d_next, uint32_t *d_head,
                               aipstack_ip4_dgram *d_dgram, void *d_workspace,
                               uint64_t workspace_bytes, void *stream);
int aipstack_ip4_rx_reassemble_slotted(const void *d_base, uint64_t slot_stride,
                                       const uint32_t *d_len, uint64_t n, uint32_t max_reass_size,
                                       uint8_t *d_verdict, uint64_t *d_chunk_addr,
                                       uint32_t *d_chunk_len, uint32_t *d_next, uint32_t *d_head,
                                       aipstack_ip4_dgram *d_dgram, void *d_workspace,
                                       uint64_t workspace_bytes, void *stream);

/* ---- ICMP on receive: echo replies and Destination Unreachable as Tx segments ------------ */

/* Every ICMP message the reference sends goes through IpStack::sendIcmp4Message
 * (ip/IpStack.h:1164-1190), from two callers: the echo reply (recvIcmp4Dgram ->
 * sendIcmp4EchoReply, :1093-1162; its data is the request's ICMP data, chained in place) and
 * Destination Unreachable (sendIp4DestUnreach, :869-887, which udp/IpUdpProto.h:609-620 calls for
 * a datagram nobody accepted; its data is the received IPv4 header plus at most 8 bytes behind
 * it). In both the data is one contiguous range of the received frame, so a response is a header
 * slot plus one chunk that points into the Rx buffer: the layout aipstack_chksum_tx_fill_hsplit,
 * aipstack_chksum_batch_chain and aipstack_tx_linearise take. These calls decide per frame whether
 * a response is due and emit it; frames in, response segments out, nothing copied.
 * Stays with this call's caller: whether an unreach should be sent at all (the listener match,
 * `accepted`, the code: d_unreach_code says so per frame; aipstack_udp_rx_demux below writes that
 * array for UDP). Stays with the host: the next hop (the reference resolves it by
 * ARP, eth/EthIpIface.h; the response's Ethernet destination is the received frame's source MAC
 * and the host may overwrite those six bytes), a response above the MTU (the reference fragments
 * it: AIPSTACK_ICMP_TOO_LARGE), and datagrams that aipstack_ip4_rx_reassemble completes: a
 * fragment (verdict 3) never gets a response here. */
#define AIPSTACK_ICMP_RESPONSE_HEADER 42u /* Ethernet 14 + IPv4 20 (IHL 5) + ICMP 8 */
#define AIPSTACK_ICMP_NONE        23  /* per frame: no response */
#define AIPSTACK_ICMP_ECHO_REPLY  24
#define AIPSTACK_ICMP_UNREACH     25
#define AIPSTACK_ICMP_TOO_LARGE   26  /* a response is due but 28 + data > mtu: the reference fragments
                                         (sendIp4Dgram, no DF); left to the host, nothing emitted, no Ident used */
#define AIPSTACK_ICMP_NO_UNREACH  0xFF /* d_unreach_code[i]: no request */
#define AIPSTACK_ICMP_ALLOW_BROADCAST_PING 1u /* iface flag: IpStackOptions::AllowBroadcastPing */

typedef struct aipstack_icmp_iface {  /* 32 bytes, host-made, host byte order; HOST memory */
    uint32_t local_addr;   /* m_addr.addr (the interface has an address: m_have_addr) */
    uint32_t bcast_addr;   /* m_addr.bcastaddr */
    uint16_t mtu;          /* IP MTU, >= AIPSTACK_UDP_MIN_MTU */
    uint16_t ip_id;        /* Ident of the first response; response j gets ip_id + j mod 2^16
                              (m_next_id++ once per sent message, ip/IpStack.h:434) */
    uint8_t  ttl;          /* IpStackOptions::IcmpTTL (default 64) */
    uint8_t  flags;        /* AIPSTACK_ICMP_ALLOW_BROADCAST_PING */
    uint8_t  mac[6];       /* Ethernet source of the responses */
    uint8_t  reserved[12]; /* 0 */
} aipstack_icmp_iface;

/* The batch (frames as aipstack_chksum_rx_verify / _rx_verify_slotted take them, under the same
 * offsets, span and slot contracts). h_iface: HOST memory, read before the call returns.
 * d_unreach_code: NULL (no requests) or n bytes: the ICMP code of a Destination Unreachable the
 * host wants for frame i, AIPSTACK_ICMP_NO_UNREACH for none.
 *
 * Which frames get a response (src / dst = the received IPv4 addresses):
 *   echo reply  Rx verify accepts the frame (AIPSTACK_RX_ACCEPT: ICMP >= 8 bytes, checksum good,
 *               :1116, :1127), protocol 1, ICMP type 8 (the code is not looked at, :1137); src
 *               is not all-ones, not multicast ((src & 0xF0000000) == 0xE0000000) and not
 *               bcast_addr (checkUnicastSrcAddr, :838-843); dst is local_addr, or bcast_addr or
 *               all-ones with AIPSTACK_ICMP_ALLOW_BROADCAST_PING (:1103-1113, :1140).
 *   unreach     no echo reply is due; d_unreach_code[i] != 0xFF; verdict AIPSTACK_RX_ACCEPT,
 *               _ACCEPT_NO_CHKSUM or _ACCEPT_OTHER; dst == local_addr and src neither all-ones
 *               nor bcast_addr (checkSendIp4Allowed with {dst, src}, :666-690; a multicast source
 *               is not rejected there, nor here).
 * A response with 28 + data > mtu is AIPSTACK_ICMP_TOO_LARGE: nothing is emitted for it and it
 * takes no Ident here (the reference's fragmented send consumes one: the host that takes this
 * slow path advances ip_id itself).
 *
 * The response bytes, for the j-th response in frame order:
 *   Ethernet  destination = the frame's source MAC, source = mac, EtherType 0x0800;
 *   IPv4      (sendIp4Dgram, :423-453) 0x4500 (IHL 5 whatever options the request carried), total
 *             length 28 + data, Ident ip_id + j, flags / offset 0, TTL ttl, protocol 1, source =
 *             local_addr (echo) or dst (unreach: the same value), destination = src, the header
 *             checksum;
 *   ICMP      (:1171-1185) echo reply: type 0, code 0, the request's `rest` (header bytes 4-7),
 *             data = the request's ICMP data, IP-payload bytes [8, total length - 4*IHL)
 *             (Ethernet padding is not data); unreach: type 3, the host's code, rest 0, data = the
 *             received IPv4 header with its options plus the first min(8, total length - 4*IHL)
 *             bytes behind it (:878-883). Checksum = IpChksum over the 8 header bytes with the
 *             field as 0, then the data, stored as computed (a computed 0 stays 0x0000). The echo
 *             checksum follows from the verified request's field by one's-complement arithmetic
 *             except where rest + data sum to 0 mod 0xFFFF: there the reference stores 0xFFFF if
 *             all those bytes are zero and 0x0000 otherwise, and the data is read to decide.
 *
 * Outputs, all written for all n frames in every call (outputs depend on inputs only):
 *   d_verdict[i]   Rx verify's verdict, unchanged;
 *   d_status[i]    AIPSTACK_ICMP_NONE / _ECHO_REPLY / _UNREACH / _TOO_LARGE;
 *   d_hdr_len[i]   42 for a response, else 0 (aipstack_tx_linearise skips such a segment);
 *   header slots   a response's 42 bytes at d_hdr + i*hdr_stride (hdr_stride >= 42), the slot's
 *                  bytes [42, min(hdr_stride, 64)) written as 0 (a 64-byte ring on a 64-byte
 *                  boundary is stored in whole lines), bytes past 64 untouched; the slot of a
 *                  frame without a response is untouched;
 *   chunk table    compact, in the form and contract of aipstack_chksum_batch_chain: no empty
 *                  chunks; d_chunk_index has n+1 entries with steps of 0 or 1; a response with
 *                  data has one chunk, the DEVICE address of the data where it lies in the Rx
 *                  buffer and its length (an echo reply without data has none). d_chunk_addr /
 *                  d_chunk_len hold n entries each; those at and beyond d_chunk_index[n] are
 *                  written as address 0, length 0;
 *   d_response_frame  n entries: entry j = the frame index of the j-th response, entries at and
 *                  beyond the count written as ~0;
 *   d_counts[2]    [0] the number of responses, [1] the number of chunks.
 *
 * Stream-ordered launches through the caller's workspace (8-byte aligned, at least
 * aipstack_icmp_rx_respond_workspace_bytes(n) = 16 * (ceil(n / 256) + 1) bytes, free again once
 * the stream passes the call): Rx verify, unchanged; a decide pass (one frame per lane: of an
 * accepted frame at most the first 82 header bytes, never past the frame's own length; d_status;
 * per 256-frame block the number of responses and chunks); a scan of the block counts by one
 * workgroup; an emit pass (each responder's slot, table entry and list entry at its place in
 * frame order; the tails of the lists). No kernel waits for another workgroup. Never allocates or
 * synchronises; can be captured into a graph and repeated. _EINVAL before any work for a null
 * pointer other than d_unreach_code, hdr_stride < 42, mtu < 256, a flag bit other than
 * _ALLOW_BROADCAST_PING, a reserved byte that is not 0, n > 2^40, d_chunk_addr / d_chunk_index /
 * d_response_frame / d_counts or the workspace not 8-byte aligned, d_hdr_len / d_chunk_len not
 * 4-byte aligned, a short workspace, a slot stride outside (0, AIPSTACK_CHKSUM_MAX_SLOT_STRIDE];
 * n == 0 is a no-op. */
uint64_t aipstack_icmp_rx_respond_workspace_bytes(uint64_t n);
int aipstack_icmp_rx_respond(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                             const aipstack_icmp_iface *h_iface, const uint8_t *d_unreach_code,
                             uint8_t *d_verdict, uint8_t *d_status, void *d_hdr,
                             uint64_t hdr_stride, uint32_t *d_hdr_len, uint64_t *d_chunk_addr,
                             uint32_t *d_chunk_len, uint64_t *d_chunk_index,
                             uint64_t *d_response_frame, uint64_t *d_counts, void *d_workspace,
                             uint64_t workspace_bytes, void *stream);
int aipstack_icmp_rx_respond_slotted(const void *d_base, uint64_t slot_stride,
                                     const uint32_t *d_len, uint64_t n,
                                     const aipstack_icmp_iface *h_iface,
                                     const uint8_t *d_unreach_code, uint8_t *d_verdict,
                                     uint8_t *d_status, void *d_hdr, uint64_t hdr_stride,
                                     uint32_t *d_hdr_len, uint64_t *d_chunk_addr,
                                     uint32_t *d_chunk_len, uint64_t *d_chunk_index,
                                     uint64_t *d_response_frame, uint64_t *d_counts,
                                     void *d_workspace, uint64_t workspace_bytes, void *stream);

/* ---- UDP Rx demux: associations, listeners and port unreachable of a batch of frames ------ */

/* What the reference does with a UDP datagram between its length check and the calls of the
 * handlers (IpUdpProto::recvIp4Dgram, udp/IpUdpProto.h:470-621): read the ports, truncate the
 * datagram to the UDP length (:492), look up the association (:527-537), walk the listener list
 * with incomingPacketMatches (:255-289) and decide to send a port unreachable (:611-619) -- for a
 * batch of frames in device memory. (The section stands behind the ICMP one because it takes its
 * aipstack_icmp_iface; it continues the TCP Rx parse, whose key table and sort it shares.) The
 * host's UDP Rx loop becomes "for each entry of d_deliver_frame: call the handlers the record
 * names", and d_unreach_code goes to aipstack_icmp_rx_respond as it is.
 * Stays with the host: calling the handlers and what they return (AcceptStop ends the walk;
 * a host whose handlers all return Reject sets the frame's unreach code itself); updateCachedInfo
 * after a callback that changes the interface address (:503-506, :560, :606: a host that does
 * that re-evaluates the rest of that frame itself); the IP-level interface listeners of
 * ip/IpStack.h:1059-1067; more than 64 listeners; datagrams that aipstack_ip4_rx_reassemble
 * completes (a fragment, verdict 3, gets no record here). */
#define AIPSTACK_UDP_NO_ASSOC        0xFFFFFFFFu
#define AIPSTACK_UDP_ASSOC_NONLOCAL  0x80000000u /* table cookie bit 31: UdpAssociationParams::accept_nonlocal_dst */
#define AIPSTACK_UDP_MAX_LISTENERS   64u
#define AIPSTACK_UDP_LIS_BROADCAST   1u          /* UdpListenParams::accept_broadcast */
#define AIPSTACK_UDP_LIS_NONLOCAL    2u          /* UdpListenParams::accept_nonlocal_dst */
#define AIPSTACK_UDP_DGRAM_VALID        0x80u
#define AIPSTACK_UDP_DGRAM_HAS_CHKSUM   1u       /* UdpRxInfo::has_checksum (:637) */
#define AIPSTACK_UDP_DGRAM_DST_LOCAL    2u       /* dst_is_iface_addr (:504) */
#define AIPSTACK_UDP_DGRAM_DST_BCAST    4u       /* is_bcast (:270-272) */

typedef struct aipstack_udp_listener {  /* 16 bytes; DEVICE table, in the order the reference iterates
                                           m_listeners_list (startListening prepends: newest first) */
    uint32_t iface_addr;                /* UdpListenParams::iface_addr, 0 = any */
    uint16_t port;                      /* 0 = any */
    uint8_t  flags;                     /* AIPSTACK_UDP_LIS_* */
    uint8_t  reserved0;                 /* 0 */
    uint32_t cookie;                    /* the caller's handle; not read by the device */
    uint32_t reserved1;                 /* 0 */
} aipstack_udp_listener;

typedef struct aipstack_udp_rx_dgram {  /* 32 bytes, host byte order; all zero unless _VALID */
    uint32_t remote_addr, local_addr;   /* IPv4 source, destination */
    uint16_t remote_port, local_port;   /* UDP source, destination */
    uint16_t data_off;                  /* 14 + 4*IHL + 8, from the frame start */
    uint16_t data_len;                  /* UDP length - 8 (:492), not the IPv4 length, not the frame's */
    uint64_t listeners;                 /* bit k: listener k matches (incomingPacketMatches) */
    uint32_t assoc;                     /* cookie & 0x7FFFFFFF of the eligible association, else _NO_ASSOC */
    uint8_t  flags;                     /* AIPSTACK_UDP_DGRAM_* */
    uint8_t  ttl;                       /* IpRxInfoIp4::ttl */
    uint16_t reserved;                  /* 0 */
} aipstack_udp_rx_dgram;

/* The batch (frames as aipstack_chksum_rx_verify / _rx_verify_slotted take them, under the same
 * offsets, span and slot contracts) comes from one interface, h_iface (HOST memory, read before
 * the call returns; validated as aipstack_icmp_rx_respond validates it, because the same struct
 * goes there next; only local_addr and bcast_addr are used here).
 * d_assocs: n_assocs aipstack_tcp_pcb_key entries in DEVICE memory, {local_addr, remote_addr,
 * local_port, remote_port} = UdpAssociationKey, sorted by aipstack_tcp_pcb_table_sort
 * (AssociationKeyCompare, :436-441, has the field order of TcpPcbKeyCompare), keys unique; the
 * cookie's low 31 bits are the caller's handle, bit 31 is accept_nonlocal_dst (n_assocs == 0: no
 * table, d_assocs may be NULL). An unsorted table gives unspecified assoc values (and with them
 * unspecified unreach codes and deliveries of the frames concerned), never an access outside the
 * table.
 * d_listeners: n_listeners <= 64 entries in DEVICE memory: the listeners whose `iface` parameter
 * is null or is this interface (:266), in list order, so that bit k of a record names entry k
 * (n_listeners == 0: d_listeners may be NULL). An entry is read by its defined bits only: set
 * reserved bytes or other flag bits change nothing; the device does not validate the tables.
 * Per frame i (src / dst = the received IPv4 addresses):
 *   - d_verdict[i]: Rx verify's verdict, unchanged;
 *   - d_dgrams[i]: a VALID record for verdict AIPSTACK_RX_ACCEPT or _ACCEPT_NO_CHKSUM with
 *     protocol 17 (Rx verify has applied the length checks of :473-489; they are applied again so
 *     that every read lies inside the frame); 32 zero bytes for every other frame. In it:
 *     dst_local = (dst == local_addr); is_bcast = (dst == 0xFFFFFFFF || dst == bcast_addr);
 *     has_checksum = the checksum field is not 0;
 *     assoc: the association is the entry equal to {dst, src, dst port, src port}; it is eligible
 *     when found and (cookie bit 31 set or dst_local) (:535), else assoc is _NO_ASSOC;
 *     listeners bit k (:262-288): (port == 0 or port == dst port) and not (is_bcast without
 *     _LIS_BROADCAST) and not (neither _LIS_NONLOCAL nor is_bcast nor dst_local) and (iface_addr
 *     == 0 or iface_addr == the interface's local_addr);
 *   - d_unreach_code[i]: 3 (Icmp4Code::DestUnreachPortUnreach) for a valid record with dst_local,
 *     no eligible association and no matching listener (:611-619 with no handler ever called),
 *     AIPSTACK_ICMP_NO_UNREACH for every other frame; written for all n frames. The source checks
 *     of checkSendIp4Allowed stay in aipstack_icmp_rx_respond.
 *   - d_deliver_frame: n entries: the indices of the frames with an eligible association or a
 *     matching listener, in frame order; the entries at and beyond the count written as ~0;
 *   - d_counts[2]: [0] the number of deliveries, [1] the number of code-3 requests.
 * Stream-ordered launches through the caller's workspace (8-byte aligned, at least
 * aipstack_udp_rx_demux_workspace_bytes(n) = 16 * (ceil(n / 256) + 1) + 32 * ceil(n / 256) bytes,
 * free again once the stream passes the call): Rx verify, unchanged; a demux pass (one frame per
 * lane: the listener table once per workgroup; of a frame accepted as UDP at most the first 82
 * header bytes, never past the frame's own length; the records, the codes; per 256-frame block
 * the number of deliveries and of requests and the delivery bits); a scan of the block counts by
 * one workgroup; an emit pass (d_deliver_frame and its tail). No kernel waits for another
 * workgroup. Never allocates or synchronises; can be captured into a graph and repeated (outputs
 * depend on inputs only; every output is written for all n frames). _EINVAL before any work for
 * a null pointer (but d_assocs with n_assocs == 0, d_listeners with n_listeners == 0), n or
 * n_assocs above 2^40, n_listeners > 64, an interface aipstack_icmp_rx_respond rejects, d_dgrams
 * / d_deliver_frame / d_counts / a table / the workspace not 8-byte aligned, a short workspace,
 * a slot stride outside (0, AIPSTACK_CHKSUM_MAX_SLOT_STRIDE]; n == 0 is a no-op. */
uint64_t aipstack_udp_rx_demux_workspace_bytes(uint64_t n);
int aipstack_udp_rx_demux(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                          const aipstack_icmp_iface *h_iface,
                          const aipstack_tcp_pcb_key *d_assocs, uint64_t n_assocs,
                          const aipstack_udp_listener *d_listeners, uint32_t n_listeners,
                          uint8_t *d_verdict, aipstack_udp_rx_dgram *d_dgrams,
                          uint8_t *d_unreach_code, uint64_t *d_deliver_frame, uint64_t *d_counts,
                          void *d_workspace, uint64_t workspace_bytes, void *stream);
int aipstack_udp_rx_demux_slotted(const void *d_base, uint64_t slot_stride, const uint32_t *d_len,
                                  uint64_t n, const aipstack_icmp_iface *h_iface,
                                  const aipstack_tcp_pcb_key *d_assocs, uint64_t n_assocs,
                                  const aipstack_udp_listener *d_listeners, uint32_t n_listeners,
                                  uint8_t *d_verdict, aipstack_udp_rx_dgram *d_dgrams,
                                  uint8_t *d_unreach_code, uint64_t *d_deliver_frame,
                                  uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes,
                                  void *stream);

/* ---- ARP on receive: replies and sender mappings of a batch of frames ---------------------- */

/* The other branch of EthIpIface::recvFrame (eth/EthIpIface.h:367-390): recvArpPacket (:474-508)
 * with the address tests of save_hw_addr / get_arp_entry (:587-627, :664-698) and the reply of
 * send_arp_packet (:774-803), for a batch of frames in device memory. Every frame that Rx verify
 * calls AIPSTACK_RX_DROP_NOT_IP4 because its EtherType is 0x0806 gets a 16-byte record that says
 * what the host's ARP table has to do with its sender, and a request for the interface's address
 * gets its 42-byte reply as a header slot without any chunk, which aipstack_tx_linearise turns
 * into a frame. ARP carries no checksum, so these calls do not run Rx verify.
 * Stays with the host: the ARP table itself (the LRU list, weak and hard entries, recycling,
 * timers, the Query and Refreshing states, the retry lists, resolve_hw_addr and the requests it
 * sends) and the observers' callbacks. */
#define AIPSTACK_ARP_REPLY_HEADER 42u /* Ethernet 14 + ARP 28 */
#define AIPSTACK_ARP_NONE       27  /* per frame: shorter than 14 bytes, or EtherType != 0x0806 (:370, :387) */
#define AIPSTACK_ARP_MALFORMED  28  /* ARP, but shorter than 14 + 28 (:477), or HwType != 1, ProtoType !=
                                       0x0800, HwAddrLen != 6 or ProtoAddrLen != 4 (:483-489) */
#define AIPSTACK_ARP_SEEN       29  /* a valid ARP packet, no reply due */
#define AIPSTACK_ARP_REPLY      30  /* a valid ARP packet, reply emitted */
#define AIPSTACK_ARP_HAVE_ADDR  1u  /* iface flag: the interface has an address (getIp4Addrs() != nullptr) */
#define AIPSTACK_ARP_REC_LEARN  1u  /* the sender MAC is not ff:ff:ff:ff:ff:ff: save_hw_addr goes on to
                                       get_arp_entry (:590) */
#define AIPSTACK_ARP_REC_NEW_OK 2u  /* get_arp_entry may create an entry for the sender address (:675-698) */
#define AIPSTACK_ARP_REC_NOTIFY 4u  /* the observers are notified (:622) */
#define AIPSTACK_ARP_REC_REPLY  8u  /* a reply was emitted (status AIPSTACK_ARP_REPLY) */

typedef struct aipstack_arp_iface {  /* 32 bytes, host-made, host byte order; HOST memory */
    uint32_t local_addr;   /* m_addr.addr; not looked at without AIPSTACK_ARP_HAVE_ADDR */
    uint32_t netmask;      /* m_addr.netmask; netaddr = local_addr & netmask and bcastaddr =
                              netaddr | ~netmask, as IpIface::setIp4Addr derives them */
    uint8_t  mac[6];       /* the interface's MAC: Ethernet source and sender of the replies */
    uint8_t  flags;        /* AIPSTACK_ARP_HAVE_ADDR */
    uint8_t  reserved[17]; /* 0 */
} aipstack_arp_iface;

typedef struct aipstack_arp_record {  /* 16 bytes; all zero but `status` for _ARP_NONE / _ARP_MALFORMED */
    uint32_t sender_addr;   /* SrcProtoAddr, host byte order */
    uint8_t  sender_mac[6]; /* SrcHwAddr, as on the wire */
    uint16_t op;            /* OpType as received, host byte order (any value; only 1 is looked at) */
    uint8_t  flags;         /* AIPSTACK_ARP_REC_* */
    uint8_t  status;        /* AIPSTACK_ARP_*: d_status[i] */
    uint16_t reserved;      /* 0 */
} aipstack_arp_record;

/* The batch (frames as aipstack_chksum_rx_verify / _rx_verify_slotted take them, under the same
 * offsets, span and slot contracts, a slot's length clamped to min(slot_stride, 65535)) comes
 * from one interface, h_iface (HOST memory, read before the call returns). Of a frame at most
 * the first 42 bytes are read, and never a byte past the frame's own length.
 * Per frame i, with the ARP fields at frame bytes 14-41:
 *   - d_status[i]: AIPSTACK_ARP_NONE / _MALFORMED / _SEEN / _REPLY as defined above.
 *   - d_arp[i]: the record. For _SEEN / _REPLY, with ip = sender_addr:
 *       LEARN   sender_mac is not all-ones;
 *       NEW_OK  ip is neither all-ones nor zero, AIPSTACK_ARP_HAVE_ADDR is set, (ip & netmask) ==
 *               netaddr and ip != bcastaddr: what get_arp_entry asks of an address it has no
 *               entry for. It is set whatever LEARN says. The host applies a LEARN record as
 *               "an entry for ip was found, or NEW_OK": then the entry becomes Valid with
 *               sender_mac (:599-616);
 *       NOTIFY  LEARN and ip is neither all-ones nor zero, with or without an interface address
 *               (DHCP's case, :618-626);
 *       REPLY   the status is _REPLY.
 *   - a reply is due (:500-506) when OpType == 1, AIPSTACK_ARP_HAVE_ADDR is set and DstProtoAddr
 *     == local_addr, whatever LEARN says. Its 42 bytes (send_arp_packet(Reply, src_mac,
 *     src_ip_addr)) go to d_hdr + i*hdr_stride: Ethernet destination = the ARP sender hardware
 *     address (not the frame's Ethernet source), Ethernet source = mac, EtherType 0x0806; HwType
 *     1, ProtoType 0x0800, HwAddrLen 6, ProtoAddrLen 4, OpType 2, SrcHwAddr = mac, SrcProtoAddr =
 *     local_addr, DstHwAddr / DstProtoAddr = the request's sender. The slot's bytes [42,
 *     min(hdr_stride, 64)) are written as 0 (a 64-byte ring on a 64-byte boundary is stored in
 *     whole lines), bytes past 64 are untouched; the slot of a frame without a reply is
 *     untouched. No padding to 60 bytes (the reference sends 42).
 *   - d_hdr_len[i]: 42 for a reply, else 0 (aipstack_tx_linearise skips such a segment).
 *   - d_reply_frame: n entries: the frame indices of the replies in frame order, the entries at
 *     and beyond the count written as ~0;
 *   - d_seen_frame: n entries: the indices of the frames with status _SEEN or _REPLY in frame
 *     order (the records the host's table loop visits), the tail written as ~0;
 *   - d_counts[2]: [0] the number of replies, [1] the number of seen frames;
 *   - d_chunk_index[0..n]: n+1 entries, all written as 0: a reply has no chunk. d_hdr, hdr_stride,
 *     d_hdr_len and d_chunk_index go to aipstack_tx_linearise / _slotted as they are (d_status may
 *     be its d_seg_status); for its d_chunk_addr and d_chunk_len the caller passes any non-null
 *     pointers, for instance d_chunk_index itself: with an index of zeros no entry of either
 *     array is ever read.
 * Every output is written for all n frames in every call, and outputs depend on inputs only.
 * Stream-ordered launches through the caller's workspace (8-byte aligned, at least
 * aipstack_arp_rx_respond_workspace_bytes(n) = 16 * (ceil(n / 256) + 1) + 64 * ceil(n / 256)
 * bytes, free again once the stream passes the call): a decide pass (one frame per lane: the
 * frame's bytes 10-33 and 38-41 at its own alignment, d_status, d_arp, per wave the 64-bit ballots of
 * replies and of seen frames, per 256-frame tile their counts); a scan of the tile counts by one
 * workgroup; an emit pass (the lists from the ballots, each reply from the record just written,
 * d_hdr_len, d_chunk_index, the tails). No kernel waits for another workgroup. Never allocates or
 * synchronises; can be captured into a graph and repeated. _EINVAL before any work for a null
 * pointer, hdr_stride < 42, a flag bit other than AIPSTACK_ARP_HAVE_ADDR, a reserved byte that is
 * not 0, n > 2^40, d_chunk_index / d_reply_frame / d_seen_frame / d_counts or the workspace not
 * 8-byte aligned, d_hdr_len or d_arp not 4-byte aligned (d_arp on a 16-byte boundary is stored in
 * whole lines), a short workspace, a slot stride outside (0, AIPSTACK_CHKSUM_MAX_SLOT_STRIDE];
 * n == 0 is a no-op. */
uint64_t aipstack_arp_rx_respond_workspace_bytes(uint64_t n);
int aipstack_arp_rx_respond(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                            const aipstack_arp_iface *h_iface, uint8_t *d_status,
                            aipstack_arp_record *d_arp, void *d_hdr, uint64_t hdr_stride,
                            uint32_t *d_hdr_len, uint64_t *d_chunk_index, uint64_t *d_reply_frame,
                            uint64_t *d_seen_frame, uint64_t *d_counts, void *d_workspace,
                            uint64_t workspace_bytes, void *stream);
int aipstack_arp_rx_respond_slotted(const void *d_base, uint64_t slot_stride, const uint32_t *d_len,
                                    uint64_t n, const aipstack_arp_iface *h_iface,
                                    uint8_t *d_status, aipstack_arp_record *d_arp, void *d_hdr,
                                    uint64_t hdr_stride, uint32_t *d_hdr_len,
                                    uint64_t *d_chunk_index, uint64_t *d_reply_frame,
                                    uint64_t *d_seen_frame, uint64_t *d_counts, void *d_workspace,
                                    uint64_t workspace_bytes, void *stream);

/* ---- TCP without a connection: listener match and RST replies of a batch of frames -------- */

/* What the reference does with a TCP datagram around find_pcb, short of pcb_input and of the
 * PCB allocation in listen_input: the local-address test in front (tcp/IpTcpProto_input.h:72),
 * and for a segment without a PCB checkUnicastSrcAddr (:139, ip/IpStack.h:839-843),
 * find_listener_for_rx (:145, tcp/IpTcpProto.h:824-837), the flag and MSS tests at the top of
 * listen_input (:372-401, CalcTcpSndMss, tcp/TcpMiscUtils.h:55-67) and the RST of
 * send_rst_reply / send_rst / send_tcp_nodata (tcp/IpTcpProto_output.h:989-1018, :1338-1404)
 * -- for a batch of frames in device memory. These calls do Rx verify, everything
 * aipstack_tcp_rx_parse does (the same d_verdict, d_segs and d_pcb, byte for byte), and then
 * decide per frame: the host calls pcb_input (_RSP_PCB), the host continues listen_input at
 * "check maximum number of PCBs" (:383, _RSP_SYN), nothing happens, or an RST leaves. The RST is
 * a 54-byte segment without data, emitted as a header slot without any chunk, which
 * aipstack_tx_linearise turns into a frame. The host's TCP receive loop becomes "for each
 * _RSP_PCB frame: pcb_input; for each _RSP_SYN frame: the rest of listen_input".
 * Stays with the host: everything in listen_input from :383 on (the PCB count, allocation, the
 * ISS, the SYN-ACK; a SYN the host then refuses gets its RST through d_rst_request in a later
 * call), pcb_input, the next hop of the reply (routing and ARP: the RST's Ethernet destination is
 * the received frame's source MAC and the host may overwrite those six bytes), segments that
 * aipstack_ip4_rx_reassemble completes (a fragment never gets an answer here), and more than
 * AIPSTACK_TCP_MAX_LISTENERS listeners. */
#define AIPSTACK_TCP_RSP_HEADER 54u       /* = AIPSTACK_TCP_SEGMENT_HEADER: Ethernet 14 + IPv4 20 + TCP 20 */
#define AIPSTACK_TCP_RSP_NONE       31    /* per frame: no valid segment record (not accepted as TCP, or
                                             AIPSTACK_RX_DROP_TCP_OFFSET) */
#define AIPSTACK_TCP_RSP_NOT_LOCAL  32    /* valid record, dst != local_addr (:72: dropped, PCB or not) */
#define AIPSTACK_TCP_RSP_PCB        33    /* dst local, PCB found, no RST requested: the host calls pcb_input */
#define AIPSTACK_TCP_RSP_DROP       34    /* dst local, no PCB (or an RST requested), nothing sent */
#define AIPSTACK_TCP_RSP_SYN        35    /* a listener matched a pure SYN with an acceptable MSS */
#define AIPSTACK_TCP_RSP_RST        36    /* an RST was emitted */
#define AIPSTACK_TCP_NO_LISTENER 0xFFFFFFFFu
#define AIPSTACK_TCP_MAX_LISTENERS 256u

typedef struct aipstack_tcp_listener {  /* 16 bytes; DEVICE table, in the order the reference walks
                                           m_listeners_list (listenIp4 prepends: newest first) */
    uint32_t addr;       /* the listener's address, host byte order; 0 = any */
    uint16_t port;
    uint16_t reserved0;  /* ignored */
    uint32_t cookie;     /* the caller's listener handle */
    uint32_t reserved1;  /* ignored */
} aipstack_tcp_listener;

/* The batch (frames as aipstack_chksum_rx_verify / _rx_verify_slotted take them, under the same
 * offsets, span and slot contracts) comes from one interface. h_iface: HOST memory, read before
 * the call returns, validated as aipstack_icmp_rx_respond validates it; used here: local_addr,
 * bcast_addr, mtu, ip_id, mac. Its ttl is the ICMP TTL and is not used: tcp_ttl (1..255, the
 * reference's TcpTTL, default 64) is the RSTs' TTL. d_pcbs / n_pcbs: the sorted key table of
 * aipstack_tcp_rx_parse, under the same contract. d_listeners / n_listeners: at most
 * AIPSTACK_TCP_MAX_LISTENERS entries in DEVICE memory, 8-byte aligned, read once per workgroup
 * into LDS; only addr, port and cookie influence the result (reserved0 travels with the port's
 * load and is masked off, reserved1 is never loaded; n_listeners == 0: no table, d_listeners may
 * be NULL);
 * the first entry in table order with port == dst port && (addr == dst || addr == 0) wins.
 * d_rst_request: NULL, or n bytes; nonzero = the host wants send_rst_reply for frame i whatever
 * the tables say (a SYN it refused in an earlier pass: m_num_pcbs >= m_max_pcbs, allocate_pcb
 * failed), the counterpart of d_unreach_code.
 *
 * Per frame i, with src / dst the received IPv4 addresses and flags the record's OffsetFlags:
 *   d_verdict[i], d_segs[i], d_pcb[i]   what aipstack_tcp_rx_parse writes;
 *   d_status[i]   _RSP_NONE       no valid record;
 *                 _RSP_NOT_LOCAL  dst != local_addr;
 *                 _RSP_PCB        a PCB was found and d_rst_request[i] is 0;
 *                 _RSP_DROP       src is all-ones, multicast ((src & 0xF0000000) == 0xE0000000) or
 *                                 bcast_addr; or no listener and RST set (:149); or a listener
 *                                 matched, (flags & 0x17) != 0x02 and (flags & 0x14) != 0x10
 *                                 (:372-379; SYN+FIN is among these);
 *                 _RSP_SYN        a listener matched, (flags & 0x17) == 0x02 (SYN without FIN, RST,
 *                                 ACK), and no MSS option or one >= 216 (MinAllowedMss = MinMTU -
 *                                 40; mtu - 40 >= 216 always). The options are those of the record;
 *                 _RSP_RST        the source passes and: d_rst_request[i] != 0 (no listener is
 *                                 consulted); or no listener and RST clear; or a listener matched,
 *                                 (flags & 0x17) != 0x02 and (flags & 0x14) == 0x10; or a listener
 *                                 matched a pure SYN whose MSS option is below 216.
 *   d_listener[i] the matched entry's cookie where a listener was consulted and matched (_RSP_SYN,
 *                 and the _RSP_DROP / _RSP_RST cases behind a match), else AIPSTACK_TCP_NO_LISTENER.
 *
 * The RST's 54 bytes, for the j-th RST in frame order:
 *   Ethernet  destination = the frame's source MAC, source = mac, EtherType 0x0800;
 *   IPv4      (sendIp4Dgram, ip/IpStack.h:423-453) 0x4500 (IHL 5 whatever options the segment
 *             carried), total length 40, Ident ip_id + j mod 2^16, flags / offset 0x4000
 *             (TcpIpSendFlags = DF), TTL tcp_ttl, protocol 6, source = dst, destination = src, the
 *             header checksum;
 *   TCP       ports swapped; with ACK in flags: seq = the segment's ack_num, ack 0, OffsetFlags
 *             0x5004 (RST); else seq 0, ack = seq_num + data_len + ((flags & 0x03) != 0) mod 2^32,
 *             OffsetFlags 0x5014 (RST|ACK); data_len is the record's (Ethernet padding is not
 *             data); window 0, urgent 0; the checksum over pseudo-header and header, stored as
 *             computed (a computed 0 stays 0x0000).
 * The ICMP and the TCP responder each take a start Ident: the host gives the second call ip_id +
 * the first call's response count. The reference draws both from one counter (m_next_id) in frame
 * order, so within a batch its Idents interleave differently; an Ident only has to be unique per
 * (source, destination, protocol) while a datagram may be in flight, RSTs carry DF and are never
 * fragmented, and each value is still used once.
 *
 * Outputs, all written for all n frames in every call (outputs depend on inputs only):
 *   header slots   an RST's 54 bytes at d_hdr + i*hdr_stride (hdr_stride >= 54), the slot's bytes
 *                  [54, min(hdr_stride, 64)) written as 0 (a 64-byte ring on a 64-byte boundary is
 *                  stored in whole lines), bytes past 64 untouched; the slot of a frame without an
 *                  RST is untouched;
 *   d_hdr_len[i]   54 for an RST, else 0 (aipstack_tx_linearise skips such a segment);
 *   d_chunk_index  n+1 entries, all written as 0: an RST has no chunk. d_hdr, hdr_stride, d_hdr_len
 *                  and d_chunk_index go to aipstack_tx_linearise / _slotted as ARP's replies do;
 *   d_response_frame  n entries: the frame indices of the RSTs in frame order, the entries at and
 *                  beyond the count written as ~0;
 *   d_syn_frame    the same for the _RSP_SYN frames;
 *   d_counts[2]    [0] the number of RSTs, [1] the number of _RSP_SYN frames.
 *
 * Stream-ordered launches through the caller's workspace (8-byte aligned, at least
 * aipstack_tcp_rx_respond_workspace_bytes(n) = 16 * (ceil(n / 256) + 1) + 64 * ceil(n / 256)
 * bytes, free again once the stream passes the call): Rx verify, unchanged; a decide pass (one
 * frame per lane: of a frame accepted as TCP at most the first 134 header bytes, never past the
 * frame's own length; status, record, pcb and listener; per wave the ballots of RSTs and SYNs,
 * per 256-frame tile their counts); a scan of the tile counts by one workgroup; an emit pass (the
 * lists from the ballots, each RST from the record just written and the frame's bytes 6-11,
 * d_hdr_len, d_chunk_index, the tails). No kernel waits for another workgroup. Never allocates or
 * synchronises; can be captured into a graph and repeated. _EINVAL before any work for a null
 * pointer other than d_rst_request and the two tables when their count is 0, n or n_pcbs above
 * 2^40, n_listeners > AIPSTACK_TCP_MAX_LISTENERS, tcp_ttl outside 1..255, an interface
 * aipstack_icmp_rx_respond rejects, hdr_stride < 54, d_segs / d_pcbs / d_listeners /
 * d_chunk_index / d_response_frame / d_syn_frame / d_counts or the workspace not 8-byte aligned,
 * d_pcb / d_listener / d_hdr_len not 4-byte aligned, a short workspace, a slot stride outside
 * (0, AIPSTACK_CHKSUM_MAX_SLOT_STRIDE]; n == 0 is a no-op. */
uint64_t aipstack_tcp_rx_respond_workspace_bytes(uint64_t n);
int aipstack_tcp_rx_respond(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                            const aipstack_icmp_iface *h_iface, uint32_t tcp_ttl,
                            const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                            const aipstack_tcp_listener *d_listeners, uint32_t n_listeners,
                            const uint8_t *d_rst_request, uint8_t *d_verdict,
                            aipstack_tcp_rx_seg *d_segs, uint32_t *d_pcb, uint8_t *d_status,
                            uint32_t *d_listener, void *d_hdr, uint64_t hdr_stride,
                            uint32_t *d_hdr_len, uint64_t *d_chunk_index,
                            uint64_t *d_response_frame, uint64_t *d_syn_frame, uint64_t *d_counts,
                            void *d_workspace, uint64_t workspace_bytes, void *stream);
int aipstack_tcp_rx_respond_slotted(const void *d_base, uint64_t slot_stride, const uint32_t *d_len,
                                    uint64_t n, const aipstack_icmp_iface *h_iface, uint32_t tcp_ttl,
                                    const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                                    const aipstack_tcp_listener *d_listeners, uint32_t n_listeners,
                                    const uint8_t *d_rst_request, uint8_t *d_verdict,
                                    aipstack_tcp_rx_seg *d_segs, uint32_t *d_pcb, uint8_t *d_status,
                                    uint32_t *d_listener, void *d_hdr, uint64_t hdr_stride,
                                    uint32_t *d_hdr_len, uint64_t *d_chunk_index,
                                    uint64_t *d_response_frame, uint64_t *d_syn_frame,
                                    uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes,
                                    void *stream);

/* ---- ICMP Destination Unreachable on receive: the quoted header and its TCP PCB ------------ */

/* The one ICMP type the reference acts on that aipstack_icmp_rx_respond reports as
 * AIPSTACK_ICMP_NONE: Destination Unreachable (type 3). recvIcmp4Dgram runs its source and
 * destination tests (ip/IpStack.h:1093-1148), handleIcmp4DestUnreach parses the IPv4 header quoted
 * inside the message (:1192-1249) and calls the handler of the quoted protocol; TCP's reads the
 * quoted ports and sequence number and calls find_pcb (tcp/IpTcpProto_input.h:154-182), UDP's is
 * empty. All of that is stateless; these calls do it for a batch of frames in device memory, so
 * that the host's handling of ICMP errors becomes "for each entry of d_pcb_frame: take that
 * record, apply the snd_una <= seq <= snd_nxt test and call handleIcmpPacketTooBig(remote_addr,
 * rest & 0xFFFF)" without reading a frame byte.
 * Stays with the host: canOutput(), the snd_una / snd_nxt window and con == nullptr
 * (tcp/IpTcpProto_input.h:186-193); the path-MTU cache and its max(MinMTU, mtu) / interface-MTU
 * clamp (ip/IpPathMtuCache.h:210-250); the requeue and the retransmission; a second interface;
 * messages that aipstack_ip4_rx_reassemble completes: a fragment (verdict 3) gets no record. */
#define AIPSTACK_ICMP_DU_NONE        37  /* per frame: no Destination Unreachable a handler would see */
#define AIPSTACK_ICMP_DU_PARSED      38  /* a valid record; the quoted protocol's handler returns at once */
#define AIPSTACK_ICMP_DU_TCP_NO_PCB  39  /* quoted TCP, code 4, >= 8 quoted L4 bytes: find_pcb finds nothing */
#define AIPSTACK_ICMP_DU_TCP_PCB     40  /* the same, and the PCB table holds the connection */

typedef struct aipstack_icmp_du_record {  /* 32 bytes, host byte order; all zero unless hl != 0 */
    uint32_t local_addr, remote_addr;   /* quoted IPv4 source, destination (IpRxInfoIp4 src_addr, dst_addr):
                                           the quoted source side is ours */
    uint16_t local_port, remote_port;   /* quoted L4 bytes 0-1, 2-3; 0 unless l4_len >= 8 (any protocol) */
    uint32_t seq;                       /* quoted L4 bytes 4-7; 0 unless l4_len >= 8 */
    uint32_t rest;                      /* ICMP header bytes 4-7, big-endian (Ip4DestUnreachMeta::icmp_rest);
                                           the next-hop MTU is rest & 0xFFFF (Icmp4GetMtuFromRest) */
    uint32_t pcb;                       /* the PCB's cookie, else AIPSTACK_TCP_NO_PCB */
    uint16_t ip_off;                    /* offset of the quoted IPv4 header from the frame start */
    uint16_t l4_len;                    /* dgram_initial.tot_len; the quoted L4 bytes lie at ip_off + hl */
    uint8_t  code;                      /* ICMP code (Ip4DestUnreachMeta::icmp_code) */
    uint8_t  proto, ttl, hl;            /* quoted protocol, TTL, header length (20..60) */
} aipstack_icmp_du_record;

/* The batch (frames as aipstack_chksum_rx_verify / _rx_verify_slotted take them, under the same
 * offsets, span and slot contracts) comes from one interface, h_iface (HOST memory, read before
 * the call returns; validated as aipstack_icmp_rx_respond validates it; only local_addr and
 * bcast_addr are used here). d_pcbs: n_pcbs aipstack_tcp_pcb_key entries in DEVICE memory under
 * the contract of aipstack_tcp_rx_parse: sorted by aipstack_tcp_pcb_table_sort, keys unique
 * (n_pcbs == 0: no table, d_pcbs may be NULL); an unsorted table gives unspecified pcb values (and
 * with them unspecified _DU_TCP_PCB / _DU_TCP_NO_PCB statuses, list entries and d_counts[0]),
 * never an access outside the table.
 * Per frame i (src / dst = the outer IPv4 addresses, hl / total = the outer header and total
 * length):
 *   1. the outer tests (recvIcmp4Dgram): Rx verify's verdict is AIPSTACK_RX_ACCEPT and the
 *      protocol is 1 (so ICMP has at least 8 bytes and a good checksum, :1116, :1127, and the
 *      frame is not a fragment); src is not all-ones, not multicast ((src & 0xF0000000) ==
 *      0xE0000000) and not bcast_addr (checkUnicastSrcAddr, :838-843); dst is local_addr,
 *      bcast_addr or all-ones (:1103-1113; AllowBroadcastPing gates only the echo reply, :1140);
 *      the ICMP type is 3 (the code is not tested here).
 *   2. the quoted header (handleIcmp4DestUnreach): icmp_data = IP-payload bytes [8, total - hl)
 *      (Ethernet padding is not data) has at least 20 bytes (:1196); its version nibble is 4
 *      (:1210); header_len = 4 * IHL is at least 20 and at most len(icmp_data) (:1217); the quoted
 *      total length is at least header_len (:1224). l4_len = min(len(icmp_data), quoted total
 *      length) - header_len (:1235). No other test is made: not of the quoted source against
 *      local_addr, not of the quoted fragment field, not of the quoted checksum.
 *   3. a frame that passes 1 and 2 gets the record above and a status other than _DU_NONE; every
 *      other frame gets 32 zero bytes and _DU_NONE.
 *   4. the TCP lookup: only for quoted protocol 6, code 4 (DestUnreachFragNeeded) and l4_len >= 8
 *      the table is searched for {local_addr, remote_addr, local_port, remote_port} of the record:
 *      _DU_TCP_PCB with pcb = the entry's cookie when found, _DU_TCP_NO_PCB otherwise. Every other
 *      valid record is _DU_PARSED with pcb = AIPSTACK_TCP_NO_PCB.
 * Outputs, all written for all n frames in every call (outputs depend on inputs only):
 *   d_verdict[i]   Rx verify's verdict, unchanged;
 *   d_status[i]    AIPSTACK_ICMP_DU_*;
 *   d_records[i]   the record, or 32 zero bytes;
 *   d_pcb_frame    n entries: the indices of the _DU_TCP_PCB frames in frame order, the entries at
 *                  and beyond the count written as ~0;
 *   d_counts[2]    [0] the number of _DU_TCP_PCB frames, [1] the number of valid records.
 * Stream-ordered launches through the caller's workspace (8-byte aligned, at least
 * aipstack_icmp_rx_unreach_workspace_bytes(n) = 16 * (ceil(n / 256) + 1) + 32 * ceil(n / 256)
 * bytes, free again once the stream passes the call): Rx verify, unchanged; a decide pass (one
 * frame per lane: of a frame accepted as ICMP at most the first 150 bytes, 14 + 60 + 8 + 60 + 8,
 * never past the frame's own length; the table searched from that lane, every index inside it;
 * the statuses and the records; per 256-frame block the two counts and the bits of the frames
 * with a PCB); a scan of the block counts by one workgroup; an emit pass (d_pcb_frame and its
 * tail). No kernel waits for another workgroup. Never allocates or synchronises; can be captured
 * into a graph and repeated. _EINVAL before any work for a null pointer (but d_pcbs with n_pcbs
 * == 0), n or n_pcbs above 2^40, an interface aipstack_icmp_rx_respond rejects, d_records /
 * d_pcb_frame / d_counts / d_pcbs / the workspace not 8-byte aligned, a short workspace, a slot
 * stride outside (0, AIPSTACK_CHKSUM_MAX_SLOT_STRIDE]; n == 0 is a no-op. */
uint64_t aipstack_icmp_rx_unreach_workspace_bytes(uint64_t n);
int aipstack_icmp_rx_unreach(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                             const aipstack_icmp_iface *h_iface,
                             const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                             uint8_t *d_verdict, uint8_t *d_status,
                             aipstack_icmp_du_record *d_records, uint64_t *d_pcb_frame,
                             uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes,
                             void *stream);
int aipstack_icmp_rx_unreach_slotted(const void *d_base, uint64_t slot_stride,
                                     const uint32_t *d_len, uint64_t n,
                                     const aipstack_icmp_iface *h_iface,
                                     const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                                     uint8_t *d_verdict, uint8_t *d_status,
                                     aipstack_icmp_du_record *d_records, uint64_t *d_pcb_frame,
                                     uint64_t *d_counts, void *d_workspace,
                                     uint64_t workspace_bytes, void *stream);

/* ---- Tx resolve: route, permission tests and next-hop MAC of a batch of segments ------------ */

/* The per-packet step between "a header slot holds an IPv4 header" and "the frame may leave":
 * IpStack::sendIp4Dgram's route (routeIp4, ip/IpStack.h:713-741, or routeIp4ForceIface, :764-780,
 * when the sender names an interface, as sendIcmp4Message does, :1188) and permission tests
 * (checkSendIp4Allowed, :666-690), then EthIpIface::driverSendIp4Packet's ARP lookup
 * (resolve_hw_addr, eth/EthIpIface.h:511-585, with the address tests of get_arp_entry(weak=false),
 * :635-698) and Ethernet header (:420-430). This call does it for n header slots at once, against
 * a snapshot of the interfaces and of the ARP tables in device memory.
 * Stays with the host: the ARP table's life (the LRU order, weak / hard, the timers, the Query /
 * Refreshing transitions, recycling above NumArpEntries, the retry lists), sending the ARP
 * requests, IpSendRetryRequest, the MTU test of sendIp4Dgram (:407) and FragmentationNeeded (the
 * producers fragment), the link state, more than AIPSTACK_TX_MAX_IFACES interfaces. */
#define AIPSTACK_TX_RES_NONE           41 /* per segment: nothing to resolve (below) */
#define AIPSTACK_TX_RES_SENT           42 /* bytes 0..13 of the slot are the Ethernet header: IpErr::Success */
#define AIPSTACK_TX_RES_NO_ROUTE       43 /* IpErr::NoIpRoute */
#define AIPSTACK_TX_RES_BCAST_REJECTED 44 /* IpErr::BroadcastRejected */
#define AIPSTACK_TX_RES_NONLOCAL_SRC   45 /* IpErr::NonLocalSrc */
#define AIPSTACK_TX_RES_NO_HW_ROUTE    46 /* IpErr::NoHardwareRoute */
#define AIPSTACK_TX_RES_ARP_QUERY      47 /* IpErr::ArpQueryInProgress: the entry is in Query state, or
                                             there is none and get_arp_entry would make one */
#define AIPSTACK_TX_MAX_IFACES 16u
#define AIPSTACK_TX_HAVE_ADDR    1u /* iface flag: m_have_addr */
#define AIPSTACK_TX_HAVE_GATEWAY 2u /* iface flag: m_have_gateway */
#define AIPSTACK_TX_ALLOW_BROADCAST    1u /* d_send_flags[i]: IpSendFlags::AllowBroadcastFlag */
#define AIPSTACK_TX_ALLOW_NONLOCAL_SRC 2u /* d_send_flags[i]: IpSendFlags::AllowNonLocalSrc */
#define AIPSTACK_TX_ROUTE_ANY 0xFFFFu     /* d_force_iface[i]: no interface named, routeIp4 */
#define AIPSTACK_TX_NO_ARP_ENTRY 0xFFFFFFFFu
#define AIPSTACK_ARP_STATE_QUERY      1u  /* aipstack_arp_entry.state: the values of ArpEntryState */
#define AIPSTACK_ARP_STATE_VALID      2u  /* (eth/EthIpIface.h:228); a Free entry is not in the table */
#define AIPSTACK_ARP_STATE_REFRESHING 3u
#define AIPSTACK_TX_ROUTE_GATEWAY   1u /* route flag: next_hop is the interface's gateway */
#define AIPSTACK_TX_ROUTE_BROADCAST 2u /* route flag: the MAC is ff:ff:ff:ff:ff:ff, no entry involved */
#define AIPSTACK_TX_ROUTE_NEW_ENTRY 4u /* route flag, _ARP_QUERY only: no entry exists; the host makes one
                                          in Query state and broadcasts the first request (:566-577) */
#define AIPSTACK_TX_ROUTE_FORCED    8u /* route flag: the segment named its interface */

typedef struct aipstack_tx_iface {  /* 32 bytes, host byte order; DEVICE table, 4-byte aligned, in the
                                       order m_iface_list iterates (last constructed first, IpIface.h:97) */
    uint32_t addr;                  /* m_addr.addr; ignored without _HAVE_ADDR */
    uint32_t netmask;               /* m_addr.netmask = PrefixMask(prefix); net and broadcast address are
                                       derived on the device: addr & netmask, that | ~netmask (:131-133) */
    uint32_t gateway;               /* m_gateway; ignored without _HAVE_GATEWAY */
    uint8_t  prefix;                /* m_addr.prefix, 0..32: what routeIp4 compares */
    uint8_t  flags;                 /* AIPSTACK_TX_HAVE_ADDR | AIPSTACK_TX_HAVE_GATEWAY */
    uint8_t  mac[6];                /* the interface's MAC: bytes 6..11 of a _SENT slot */
    uint8_t  reserved[12];
} aipstack_tx_iface;

typedef struct aipstack_arp_entry { /* 16 bytes, host byte order; DEVICE table, 4-byte aligned */
    uint32_t addr;                  /* ArpEntry::ip_addr */
    uint16_t iface;                 /* index into the interface table: whose ARP table this entry is of */
    uint8_t  state;                 /* AIPSTACK_ARP_STATE_*; >= _VALID resolves (:543) */
    uint8_t  mac[6];                /* ArpEntry::mac_addr; not read in Query state */
    uint8_t  reserved[3];
} aipstack_arp_entry;

typedef struct aipstack_tx_route {  /* 16 bytes, host byte order; all zero for _RES_NONE */
    uint32_t next_hop;              /* IpRouteInfoIp4::addr: the destination or the gateway; 0 for _NO_ROUTE */
    uint32_t arp_index;             /* the entry that resolved it (_SENT) or is in Query state
                                       (_ARP_QUERY), else AIPSTACK_TX_NO_ARP_ENTRY */
    uint16_t iface;                 /* IpRouteInfoIp4::iface as an index; for _NO_ROUTE the interface the
                                       segment named, or AIPSTACK_TX_ROUTE_ANY */
    uint8_t  status;                /* AIPSTACK_TX_RES_* (0 in the all-zero record) */
    uint8_t  flags;                 /* AIPSTACK_TX_ROUTE_* */
    uint8_t  reserved[4];
} aipstack_tx_route;

/* Sorts n entries in HOST memory by (iface, addr), the order the lookup searches, as
 * aipstack_tcp_pcb_table_sort does for the PCB table. _EINVAL for a null pointer with n != 0,
 * n >= 2^32 - 1, or when two entries have the same (iface, addr), a state outside 1..3, an iface >=
 * AIPSTACK_TX_MAX_IFACES or a nonzero reserved byte (the array is sorted either way). */
int aipstack_arp_table_sort(aipstack_arp_entry *h_entries, uint64_t n);

/* Segment i is the header slot at d_hdr + i * hdr_stride that the producers (aipstack_tcp_tx_segment,
 * aipstack_udp_tx_fragment), the responders (aipstack_icmp_rx_respond, aipstack_tcp_rx_respond) and
 * aipstack_chksum_tx_fill_hsplit share, d_hdr_len[i] bytes long. Of it only bytes 12..13 and the IPv4
 * source and destination address, bytes 26..33, are read, at the slot's own alignment; nothing of
 * a chunk table is.
 *   nothing to resolve (_RES_NONE): d_hdr_len[i] < 34, or d_hdr_len[i] > hdr_stride (a length
 *   aipstack_tx_linearise rejects; no byte outside a slot is ever touched), or bytes 12..13 are not
 *   08 00 (an ARP reply of aipstack_arp_rx_respond), or d_seg_status (may be NULL) holds
 *   AIPSTACK_TX_BURST_INVALID or AIPSTACK_TX_DGRAM_INVALID for it (then no slot byte is read).
 * Every other segment, with src / dst its addresses, flags = d_send_flags[i] (NULL: 0 for all; bits
 * other than the two above are ignored) and k = d_force_iface[i] (NULL: AIPSTACK_TX_ROUTE_ANY for
 * all), in the reference's order:
 *   1. the route. k == _ROUTE_ANY: over the n_ifaces interfaces in table order, an interface
 *      with an address whose subnet holds dst replaces the best so far if its prefix is longer;
 *      one that does not hold dst but has a gateway is taken only while nothing is chosen
 *      (:718-731). next_hop = dst if a subnet matched, else the chosen interface's gateway. Any other
 *      k: that interface; next_hop = dst if dst is all-ones or in its subnet, else its gateway if
 *      it has one (:769-777). Nothing chosen, or k >= n_ifaces: _NO_ROUTE.
 *   2. without _ALLOW_BROADCAST: dst all-ones, or the routed interface has an address and dst is
 *      its broadcast address: _BCAST_REJECTED (:669-679).
 *   3. without _ALLOW_NONLOCAL_SRC: the routed interface has no address or src is not it:
 *      _NONLOCAL_SRC (:681-687).
 *   4. the table is searched for (routed interface, next_hop). Found (the first test, as in
 *      get_arp_entry, :650): state >= _VALID is _SENT with the entry's MAC, else _ARP_QUERY.
 *      Not found: next_hop all-ones is _SENT to ff:ff:ff:ff:ff:ff; zero, or an interface without
 *      an address, or next_hop outside its subnet is _NO_HW_ROUTE; its broadcast address is _SENT
 *      to ff:ff:ff:ff:ff:ff; anything else _ARP_QUERY with _ROUTE_NEW_ENTRY (:675-698, :566-583).
 * d_ifaces: n_ifaces <= AIPSTACK_TX_MAX_IFACES entries in DEVICE memory (n_ifaces == 0: every
 * segment with something to resolve is _NO_ROUTE). d_arp: n_arp entries in DEVICE memory sorted by
 * aipstack_arp_table_sort, keys unique (n_arp == 0: d_arp and d_arp_used may be NULL). An
 * unsorted table or one with duplicate keys gives unspecified outcomes of step 4, never a read
 * outside [0, n_arp).
 * Outputs, all stored for all n segments (all n_arp entries) in every call, so outputs depend on
 * inputs only and the call replays from a graph:
 *   d_status[i]     AIPSTACK_TX_RES_*;
 *   d_route[i]      the record (4-byte aligned);
 *   d_send_len[i]   d_hdr_len[i] for _SENT and _RES_NONE, else 0: passed to aipstack_tx_linearise as
 *                   its d_hdr_len, held and failed segments are skipped; the caller's d_hdr_len
 *                   stays intact for the retry after the ARP answer;
 *   d_arp_used[j]   1 where entry j resolved at least one segment (_SENT through it), else 0: the
 *                   host makes it hard, moves it in the LRU list and applies the attempts_left ==
 *                   0 -> Refreshing step (:517-559);
 *   d_held_seg      n entries: the _ARP_QUERY segments in segment order, ~0 at and beyond the
 *                   count: the host starts one query per distinct (iface, next_hop) with
 *                   _ROUTE_NEW_ENTRY and queues the retry;
 *   d_failed_seg    n entries: the _NO_ROUTE, _BCAST_REJECTED, _NONLOCAL_SRC and _NO_HW_ROUTE
 *                   segments in segment order, ~0 at and beyond the count;
 *   d_counts[2]     [0] held, [1] failed segments;
 *   the header ring, for _SENT only: bytes 0..5 the MAC, 6..11 the routed interface's MAC,
 *                   12..13 08 00, stored with the widest naturally aligned stores the slot's
 *                   address allows. No other byte of the ring is stored: no byte of another slot,
 *                   none from 14 on, none of a slot's slack.
 * Stream-ordered through the caller's workspace (8-byte aligned, at least
 * aipstack_tx_resolve_workspace(n) = 16 * (ceil(n / 256) + 1) + 64 * ceil(n / 256) bytes, free again
 * once the stream passes the call): a memset of d_arp_used; a decide pass (one segment per lane,
 * the interface table once per workgroup in LDS, the ARP table searched from that lane); a scan
 * of the 256-segment blocks' counts by one workgroup; an emit pass for the two lists. No kernel
 * waits for another workgroup. Never allocates or synchronises; can be captured into a graph.
 * flags: no bit is defined; ignored. _EINVAL before any work for a null pointer (d_seg_status,
 * d_send_flags, d_force_iface excepted, and d_arp / d_arp_used with n_arp == 0), n_ifaces >
 * AIPSTACK_TX_MAX_IFACES, hdr_stride == 0, n > 2^40, n_arp >= 2^32 - 1 (arp_index has 32 bits),
 * d_hdr_len / d_send_len / d_route /
 * d_ifaces / d_arp not 4-byte aligned, d_force_iface not 2-byte aligned, d_held_seg / d_failed_seg
 * / d_counts / the workspace not 8-byte aligned, a short workspace. n == 0 returns _OK before
 * the arguments are looked at. */
uint64_t aipstack_tx_resolve_workspace(uint64_t n);
int aipstack_tx_resolve(void *d_hdr, uint64_t hdr_stride, const uint32_t *d_hdr_len, uint64_t n,
                        const uint8_t *d_seg_status, const uint8_t *d_send_flags,
                        const uint16_t *d_force_iface, const aipstack_tx_iface *d_ifaces,
                        uint32_t n_ifaces, const aipstack_arp_entry *d_arp, uint64_t n_arp,
                        uint8_t *d_status, aipstack_tx_route *d_route, uint32_t *d_send_len,
                        uint8_t *d_arp_used, uint64_t *d_held_seg, uint64_t *d_failed_seg,
                        uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes,
                        uint32_t flags, void *stream);

/* ---- 3. host-memory streaming engine ----------------------------------------------- */

/* The reference's packet path starts and ends in host memory (TAP read()/write(),
 * reference tap/linux/TapDeviceLinux.cpp:122-178). An engine checksums batches held in
 * HOST memory and writes the results to HOST memory, pipelining H2D copies, kernels and
 * D2H copies over `nstreams` HIP streams in chunks of at most `chunk_bytes` (0 = 64 MiB)
 * of whole packets. Host buffers registered with aipstack_chksum_engine_register()
 * (page-locked once, e.g. a receive ring) are read by the kernels where they lie, over the
 * link (only the bytes the packets cover cross it: for ring slots not the slack); with
 * aipstack_chksum_tune("engine_zero_copy", 0) before the engine is created they are DMA'd
 * to the device first instead. Other host memory is first copied into the engine's pinned
 * staging (a ring of slots: each frame's bytes only, read there by the kernel; tune
 * "engine_pageable_rows" 0 = whole slots, DMA'd). The host_* calls are synchronous; the submit_*
 * calls enqueue a batch and return a ticket at once, so the caller can fill its next batch
 * (e.g. read() frames into its ring) while the GPU works; _poll / _wait complete it. Calls
 * on one engine from several threads are serialised, except that _wait waits for the GPU
 * without holding the engine: _poll and _submit_* from other threads proceed meanwhile (a
 * _submit_* that needs a busy stream still waits for the piece on it).
 *
 * Errors are per batch: a piece that fails records its status against its own ticket,
 * whichever call completes it, and _poll / _wait of that ticket return it (once). Destroy
 * completes every piece still in flight as _wait would -- results written, Tx fields
 * applied -- before freeing anything; so does _unregister before it unpins the region. */
typedef struct aipstack_chksum_engine aipstack_chksum_engine;

int aipstack_chksum_engine_create(int device, uint64_t chunk_bytes, int nstreams,
                                  aipstack_chksum_engine **out);
void aipstack_chksum_engine_destroy(aipstack_chksum_engine *engine);
int aipstack_chksum_engine_register(aipstack_chksum_engine *engine, void *host_ptr,
                                    uint64_t bytes);
int aipstack_chksum_engine_unregister(aipstack_chksum_engine *engine, void *host_ptr);

/* h_out[i] for packet i = h_base[i*stride .. +len) (host memory), as the strided batch. */
int aipstack_chksum_engine_host_strided(aipstack_chksum_engine *engine, const void *h_base,
                                        uint64_t stride, uint32_t len, uint64_t n,
                                        uint16_t *h_out, uint32_t flags);

/* h_out[i] for packet i = h_base[h_offsets[i] .. h_offsets[i+1]) (host memory; offsets
 * non-decreasing, each packet <= 65535 bytes, else _EINVAL before any work). */
int aipstack_chksum_engine_host_csr(aipstack_chksum_engine *engine, const void *h_base,
                                    const uint64_t *h_offsets, uint64_t n, uint16_t *h_out,
                                    uint32_t flags);

/* Asynchronous form of the two calls above: enqueue the batch and return at once with
 * *ticket set. h_out is written when the batch completes; a REGISTERED h_base must stay
 * unchanged until then (it is DMA'd while the GPU runs), pageable input is copied before
 * the call returns. At most nstreams chunks are in flight per engine: a submit that needs
 * a busy stream first completes the piece on it. Returns _OK or a negative status (a
 * failure part-way leaves the pieces already enqueued to _wait). */
int aipstack_chksum_engine_submit_strided(aipstack_chksum_engine *engine, const void *h_base,
                                          uint64_t stride, uint32_t len, uint64_t n,
                                          uint16_t *h_out, uint32_t flags, uint64_t *ticket);
int aipstack_chksum_engine_submit_csr(aipstack_chksum_engine *engine, const void *h_base,
                                      const uint64_t *h_offsets, uint64_t n, uint16_t *h_out,
                                      uint32_t flags, uint64_t *ticket);

/* Rx verify of raw Ethernet frames held in HOST memory -- the TAP receive path
 * (tap/linux/TapDeviceLinux.cpp:156-178) batched: h_verdicts[i] = the AIPSTACK_RX_* verdict
 * of frame i = h_base[h_offsets[i] .. h_offsets[i+1]), as aipstack_chksum_rx_verify
 * (offsets non-decreasing, each frame <= 65535 bytes, else _EINVAL before any work).
 * Synchronous and submit forms, as above. */
int aipstack_chksum_engine_host_rx_verify(aipstack_chksum_engine *engine, const void *h_base,
                                          const uint64_t *h_offsets, uint64_t n,
                                          uint8_t *h_verdicts);
int aipstack_chksum_engine_submit_rx_verify(aipstack_chksum_engine *engine, const void *h_base,
                                            const uint64_t *h_offsets, uint64_t n,
                                            uint8_t *h_verdicts, uint64_t *ticket);

/* Tx fill of raw Ethernet frames held in HOST memory -- the TAP send path batched
 * (tap/linux/TapDeviceLinux.cpp:122-127): the frames go to the device, the Tx fill's read
 * pass computes each frame's record (aipstack_chksum_tx_fill_records), 8 bytes per frame come
 * back, and the engine writes the IPv4 header and L4 checksum fields into the caller's
 * frames IN PLACE and h_status[i] (as aipstack_chksum_tx_fill) when the batch completes (poll
 * or wait). A submitted batch's frames, offsets and statuses must stay valid until then (or
 * until the engine is destroyed, which completes it). */
int aipstack_chksum_engine_host_tx_fill(aipstack_chksum_engine *engine, void *h_base,
                                        const uint64_t *h_offsets, uint64_t n,
                                        uint8_t *h_status);
int aipstack_chksum_engine_submit_tx_fill(aipstack_chksum_engine *engine, void *h_base,
                                          const uint64_t *h_offsets, uint64_t n,
                                          uint8_t *h_status, uint64_t *ticket);

/* The same three on a ring of slots in HOST memory (layout as aipstack_chksum_batch_slotted:
 * frame i is the h_len[i] bytes at h_base + i*slot_stride; the buffer holds n whole slots;
 * every h_len[i] <= min(slot_stride, 65535) and slot_stride <= chunk_bytes, else _EINVAL
 * before any work). Pieces are runs of whole slots, copied as they lie (slack included). */
int aipstack_chksum_engine_host_slotted(aipstack_chksum_engine *engine, const void *h_base,
                                        uint64_t slot_stride, const uint32_t *h_len, uint64_t n,
                                        uint16_t *h_out, uint32_t flags);
int aipstack_chksum_engine_submit_slotted(aipstack_chksum_engine *engine, const void *h_base,
                                          uint64_t slot_stride, const uint32_t *h_len, uint64_t n,
                                          uint16_t *h_out, uint32_t flags, uint64_t *ticket);
int aipstack_chksum_engine_host_rx_verify_slotted(aipstack_chksum_engine *engine,
                                                  const void *h_base, uint64_t slot_stride,
                                                  const uint32_t *h_len, uint64_t n,
                                                  uint8_t *h_verdicts);
int aipstack_chksum_engine_submit_rx_verify_slotted(aipstack_chksum_engine *engine,
                                                    const void *h_base, uint64_t slot_stride,
                                                    const uint32_t *h_len, uint64_t n,
                                                    uint8_t *h_verdicts, uint64_t *ticket);
int aipstack_chksum_engine_host_tx_fill_slotted(aipstack_chksum_engine *engine, void *h_base,
                                                uint64_t slot_stride, const uint32_t *h_len,
                                                uint64_t n, uint8_t *h_status);
int aipstack_chksum_engine_submit_tx_fill_slotted(aipstack_chksum_engine *engine, void *h_base,
                                                  uint64_t slot_stride, const uint32_t *h_len,
                                                  uint64_t n, uint8_t *h_status,
                                                  uint64_t *ticket);

/* Completion of a submitted batch: 0 = done (h_out holds the results), 1 = still running
 * (poll only), negative = one of its pieces failed (the first failure's status; h_out /
 * the frames of the failed pieces are not written), or _EINVAL for a ticket never issued.
 * _wait blocks. A ticket's failure is reported once; completing it again returns 0. */
int aipstack_chksum_engine_poll(aipstack_chksum_engine *engine, uint64_t ticket);
int aipstack_chksum_engine_wait(aipstack_chksum_engine *engine, uint64_t ticket);

/* Where the engine's host threads run: the NUMA node of its device (-1 unknown) and how many
 * of the CPUs next to the device (sysfs local_cpulist, within this process's affinity) its
 * host threads are pinned to (0 = not pinned). Its pinned staging is allocated from them. */
int aipstack_chksum_engine_locality(const aipstack_chksum_engine *engine, int *numa_node,
                                    int *pinned_cpus);
/* 1 if the engine's kernels read the registered region holding host_ptr in place (zero copy),
 * 0 if it is DMA'd to the device first, _EINVAL if host_ptr is in no registered region. */
int aipstack_chksum_engine_region_mapped(aipstack_chksum_engine *engine, const void *host_ptr);

/* ---- 4. several devices in one process -------------------------------------------- */

/* The reference stack is one process on one event-loop thread (event_loop/event_loop.dox:
 * 48-50); a host batch is PCIe-bound per device (~50 GiB/s). An engine group owns one engine
 * per entry of `devices` (repeats allowed) and splits a batch into contiguous ranges of about
 * equal bytes, one per device (a batch of less than 4 MiB per device goes to fewer devices,
 * round robin, whole): disjoint packet ranges, no data exchanged between the devices.
 *
 * The submit_* calls enqueue a batch and return ONE group ticket at once; _poll / _wait
 * complete it: 0 = done, 1 = still running (poll), else the first failure by device order;
 * dev_status (NULL or n_devices ints) then receives each device's status (0 for a device
 * without a range). A ticket is reported once: to the call that completes it and to every
 * _wait already blocked on it then; completing it again afterwards returns 0. Each range is
 * submitted to its engine on the calling thread when the batch lies in a region registered
 * with the group (the kernels read it in place) or is small, else by a persistent worker
 * thread of its device (pinned, like the engine's own host threads, to the CPUs next to the
 * device), so the pageable staging copies of all devices run in parallel while the caller
 * goes on. Every input, output and frame buffer of a submitted batch must stay valid, and its
 * input unchanged, until the ticket completes. A submit returns _OK or a negative status: the
 * argument checks fail before anything starts (*ticket = 0); a range whose engine submit fails
 * on the calling thread leaves *ticket set, the batch's other ranges running, and the failure
 * reported again by _poll / _wait, which must still complete the ticket (as for one engine).
 * The host_* calls are submit + wait.
 * _register page-locks a region once for all devices (portable, mapped into each device). */
typedef struct aipstack_chksum_engine_group aipstack_chksum_engine_group;

int aipstack_chksum_engine_group_create(const int *devices, int n_devices, uint64_t chunk_bytes,
                                        int nstreams, aipstack_chksum_engine_group **out);
void aipstack_chksum_engine_group_destroy(aipstack_chksum_engine_group *group);
int aipstack_chksum_engine_group_size(const aipstack_chksum_engine_group *group);
/* The engine of entry k (owned by the group, valid until it is destroyed), e.g. for
 * aipstack_chksum_engine_locality; NULL for k out of range. */
aipstack_chksum_engine *aipstack_chksum_engine_group_engine(aipstack_chksum_engine_group *group,
                                                            int k);
/* 1 if every engine of the group reads the group-registered region holding host_ptr in place,
 * 0 if some DMA it, _EINVAL if it is not registered with the group. */
int aipstack_chksum_engine_group_region_mapped(aipstack_chksum_engine_group *group,
                                               const void *host_ptr);
int aipstack_chksum_engine_group_register(aipstack_chksum_engine_group *group, void *host_ptr,
                                          uint64_t bytes);
int aipstack_chksum_engine_group_unregister(aipstack_chksum_engine_group *group, void *host_ptr);
int aipstack_chksum_engine_group_host_strided(aipstack_chksum_engine_group *group,
                                              const void *h_base, uint64_t stride, uint32_t len,
                                              uint64_t n, uint16_t *h_out, uint32_t flags,
                                              int *dev_status);
int aipstack_chksum_engine_group_host_csr(aipstack_chksum_engine_group *group, const void *h_base,
                                          const uint64_t *h_offsets, uint64_t n, uint16_t *h_out,
                                          uint32_t flags, int *dev_status);
int aipstack_chksum_engine_group_host_rx_verify(aipstack_chksum_engine_group *group,
                                                const void *h_base, const uint64_t *h_offsets,
                                                uint64_t n, uint8_t *h_verdicts, int *dev_status);
int aipstack_chksum_engine_group_host_tx_fill(aipstack_chksum_engine_group *group, void *h_base,
                                              const uint64_t *h_offsets, uint64_t n,
                                              uint8_t *h_status, int *dev_status);
/* Ring slots (frame i = h_len[i] bytes at h_base + i*slot_stride): contiguous runs of about
 * equal slot counts per device; every length is checked (<= min(slot_stride, 65535)) before
 * any device starts. */
int aipstack_chksum_engine_group_host_slotted(aipstack_chksum_engine_group *group,
                                              const void *h_base, uint64_t slot_stride,
                                              const uint32_t *h_len, uint64_t n, uint16_t *h_out,
                                              uint32_t flags, int *dev_status);
int aipstack_chksum_engine_group_host_rx_verify_slotted(aipstack_chksum_engine_group *group,
                                                        const void *h_base, uint64_t slot_stride,
                                                        const uint32_t *h_len, uint64_t n,
                                                        uint8_t *h_verdicts, int *dev_status);
int aipstack_chksum_engine_group_host_tx_fill_slotted(aipstack_chksum_engine_group *group,
                                                      void *h_base, uint64_t slot_stride,
                                                      const uint32_t *h_len, uint64_t n,
                                                      uint8_t *h_status, int *dev_status);
int aipstack_chksum_engine_group_submit_strided(aipstack_chksum_engine_group *group,
                                                const void *h_base, uint64_t stride, uint32_t len,
                                                uint64_t n, uint16_t *h_out, uint32_t flags,
                                                uint64_t *ticket);
int aipstack_chksum_engine_group_submit_csr(aipstack_chksum_engine_group *group,
                                            const void *h_base, const uint64_t *h_offsets,
                                            uint64_t n, uint16_t *h_out, uint32_t flags,
                                            uint64_t *ticket);
int aipstack_chksum_engine_group_submit_rx_verify(aipstack_chksum_engine_group *group,
                                                  const void *h_base, const uint64_t *h_offsets,
                                                  uint64_t n, uint8_t *h_verdicts, uint64_t *ticket);
int aipstack_chksum_engine_group_submit_tx_fill(aipstack_chksum_engine_group *group, void *h_base,
                                                const uint64_t *h_offsets, uint64_t n,
                                                uint8_t *h_status, uint64_t *ticket);
int aipstack_chksum_engine_group_submit_slotted(aipstack_chksum_engine_group *group,
                                                const void *h_base, uint64_t slot_stride,
                                                const uint32_t *h_len, uint64_t n, uint16_t *h_out,
                                                uint32_t flags, uint64_t *ticket);
int aipstack_chksum_engine_group_submit_rx_verify_slotted(aipstack_chksum_engine_group *group,
                                                          const void *h_base, uint64_t slot_stride,
                                                          const uint32_t *h_len, uint64_t n,
                                                          uint8_t *h_verdicts, uint64_t *ticket);
int aipstack_chksum_engine_group_submit_tx_fill_slotted(aipstack_chksum_engine_group *group,
                                                        void *h_base, uint64_t slot_stride,
                                                        const uint32_t *h_len, uint64_t n,
                                                        uint8_t *h_status, uint64_t *ticket);
int aipstack_chksum_engine_group_poll(aipstack_chksum_engine_group *group, uint64_t ticket,
                                      int *dev_status);
int aipstack_chksum_engine_group_wait(aipstack_chksum_engine_group *group, uint64_t ticket,
                                      int *dev_status);

/* ---- diagnostics ------------------------------------------------------------------ */

/* Contract violations the kernels met on a device since the last clear (sticky bits). The
 * batch calls never fault on inputs outside their contract, but their results for the
 * offending packets are unspecified; these bits say that it happened:
 *   _PACKET_LEN  a CSR packet or frame longer than 65535 bytes, or offsets decreasing (its
 *                result: the exact sum up to 2^26 bytes, else 0; frames: NOT_IP4)
 *   _CHUNK_LEN   a chain chunk longer than 65535 bytes (summed as an empty chunk)
 *   _SPAN        64 consecutive frames spanning more than 4 MiB (their headers read as 0)
 * aipstack_chksum_contract_violations synchronises the whole device (hipDeviceSynchronize:
 * every stream of every engine on it waits), then stores the bits in *mask and, if `clear` is
 * non-zero, clears them in the same atomic exchange (a bit set meanwhile is never lost). */
#define AIPSTACK_CHKSUM_VIOLATION_PACKET_LEN 1u
#define AIPSTACK_CHKSUM_VIOLATION_CHUNK_LEN  2u
#define AIPSTACK_CHKSUM_VIOLATION_SPAN       4u
int aipstack_chksum_contract_violations(int device, uint32_t *mask, int clear);

/* Static description of a status code. Never NULL. */
const char *aipstack_chksum_strerror(int status);

/* hipError_t of the most recent failing HIP call made by this library on the calling
 * thread (0 if none). */
int aipstack_chksum_last_hip_error(void);

/* AIPSTACK_CHKSUM_OK if `device` is a gfx950 device this library can launch on,
 * else _ENODEV (or _EHIP if the HIP runtime itself fails). */
int aipstack_chksum_device_check(int device);

/* Launch tunables, for benchmark sweeps (0 = automatic). Keys: "waves_per_cu",
 * "chunks_per_wave", "stream" (1 KiB windows a wave issues together in stream mode -- a
 * 64-packet or 64-frame chunk that lies back to back in memory, or chain chunks that lie close
 * together: 2, 4, 8; -1 turns stream mode off, so every packet, frame or chunk is summed on its
 * own), "chunk_packets" (packets, frames or chains per wave chunk: 1, 2, 4, ..., 64; automatic
 * = short runs of about 12 KiB, 64 for stream mode (ring slots 8, chains 32), fewer for small
 * batches so that they spread over more waves), "tx_gather" (where the Tx fills take their
 * header segments: 0 per-lane loads, 1 captured from the stream, 2 captured + the two field
 * lines touched up front; -1 = by kind of launch), "tx_store" (how the in-place Tx fills write
 * the two checksum fields: 0 = 2-byte stores, 1 = the fields' whole 32-byte sectors from the
 * header bytes the kernel holds, 2 = a send ring's (slots on the 128-byte grid) first 128-byte
 * line per frame written whole; -1 = the default, 0), "chain_short" (chained batches: chunks of
 * at most this many bytes that share no 128-byte line with their neighbours in the table are
 * read first in each 64-chunk group; 0 = the table's order, -1 = the default, 128), "gather"
 * (strided and CSR checksum batches on packets back to back: 1 = short runs, one ~12 KiB chunk
 * per wave, the default since round 5; 0 = the gathered stream of the packets' segments (round
 * 4); -1 = stream mode, one contiguous run per 64-packet chunk), "short_loads" (short runs: 0
 * stream prefixes, 1 the same through global loads, 2 column runs; -1 = by packet length, the
 * default), "lds_pad" (bytes of dynamic LDS per workgroup of the batch, chain and frame
 * kernels, which caps the workgroups per CU; -1 none, 0 the launch's own), "aux_blocks" (most
 * workgroups of a one-element-per-lane pass -- the header-split fill's two, the burst
 * segmentation's and the UDP fragmentation's plan and emit, the Rx parse, the split Tx fills'
 * scatter: 1 or more; -1 = the
 * default, 64 per CU; tests set 1 or 3 so that a small batch loops). Sweep builds only
 * (tools/build_variant.sh NAME -DAIPSTACK_ALL_VARIANTS; the product build rejects values other
 * than the default): "unroll" (segments per lane issued up front, 1..4), "packets" (packets a
 * wave keeps in flight: 1, 2, 4, 8), "nontemporal" (0/1), "frames" (frames in flight per wave
 * in Rx verify / Tx fill: 2, 4, 8). Process-wide; results never depend on them.
 * Returns _OK or _EINVAL for an unknown key or a rejected value. */
int aipstack_chksum_tune(const char *key, int value);

/* The launch shape the batch entry points pick for n packets on a device with `cus` compute
 * units (host-side query, no GPU needed; honours aipstack_chksum_tune): packets per wave
 * chunk (64, or fewer for a small batch, so that it spreads over more waves) and stream
 * windows in flight per wave, for the strided (csr = 0) or CSR (csr = 1) family.
 * Returns _OK, or _EINVAL for null outputs or cus <= 0. */
int aipstack_chksum_launch_shape(uint64_t n, int cus, int csr, uint32_t *chunk_packets,
                                 int *stream_windows);

/* ABI version of this header: bumped on any incompatible change. */
#define AIPSTACK_CHKSUM_ABI_VERSION 1
int aipstack_chksum_abi_version(void);

/* sha256 (hex) of the sources this library was built from (aipstack_amd/csrc/ *.hip, *.cpp,
 * *.cc, *.h, its Makefile, include/aipstack_amd/ *.h, concatenated in sorted path order):
 * lets a test or a deployment tell a library from a stale build. */
const char *aipstack_chksum_source_digest(void);

/* ---- TCP segments without data: SYN, SYN-ACK, ACK, FIN, RST ------------------------- */

/* The batched form of the reference's send_tcp_nodata (tcp/IpTcpProto_output.h:1337-1404) under
 * sendIp4Dgram (ip/IpStack.h:423-453), for its five callers: pcb_send_syn (the SYN and the
 * SYN-ACK, :79-122), pcb_send_empty_ack (:126-134), pcb_output_empty_fin_segment (:1149-1175)
 * and pcb_send_rst / send_rst (:137-142, :1012-1018). The host's state machine decides what to
 * send and fills one descriptor per segment; the call builds the header slot, both checksums
 * included, for aipstack_tx_resolve and aipstack_tx_linearise, as the RSTs of
 * aipstack_tcp_rx_respond are.
 *
 * A descriptor is invalid (AIPSTACK_TCP_CTL_INVALID) only if reserved0 or reserved1 is nonzero
 * or options has a bit besides AIPSTACK_TCP_OPT_MSS | AIPSTACK_TCP_OPT_WND_SCALE: its slot stays
 * untouched, d_hdr_len[i] = 0 and it takes no Ident. Flags and option subsets are not
 * restricted (send_tcp_nodata does not restrict them).
 *
 * The j-th valid descriptor in descriptor order, with olen = 4 * popcount(options) and
 * H = 54 + olen: Ethernet destination 0 (aipstack_tx_resolve writes it), source h_iface->mac,
 * EtherType 0x0800; IPv4 0x4500, total length 40 + olen, Ident h_iface->ip_id + j mod 2^16,
 * flags/offset 0x4000 (DF), TTL tcp_ttl, protocol 6, source local_addr, destination remote_addr,
 * the header checksum; TCP ports, seq, ack, OffsetFlags (5 + olen/4) << 12 | flags, window, the
 * checksum over the pseudo-header (length 20 + olen), the header and the options, stored as
 * computed (0 stays 0x0000), urgent 0; then the options as WriteTcpOptions writes them
 * (tcp/TcpOptions.h:141-157): 02 04 mss_hi mss_lo if _OPT_MSS, then 01 03 03 wnd_scale if
 * _OPT_WND_SCALE.
 *
 * Outputs, all written for all n descriptors in every call, from the inputs alone: the H bytes
 * at d_hdr + i*hdr_stride and zeros in [H, min(hdr_stride, 64)) of the slot (bytes past 64 and an
 * invalid descriptor's whole slot stay untouched); d_hdr_len[i] = H or 0; d_chunk_index[0..n] = 0
 * (no chunks); d_status[i] = AIPSTACK_TCP_CTL_EMITTED or _CTL_INVALID; d_counts[0] = emitted
 * (the host advances its Ident counter by it), d_counts[1] = invalid. d_ctl, d_hdr, d_hdr_len,
 * d_chunk_index, d_status, d_counts and d_workspace are DEVICE memory, h_iface HOST memory (read
 * before the call returns; local_addr, bcast_addr, mtu, ttl and flags are validated as
 * aipstack_icmp_rx_respond does, mac and ip_id are used). Three stream-ordered launches, no
 * allocation, no synchronisation.
 *
 * Returns _EINVAL before any work for a null pointer, hdr_stride < AIPSTACK_TCP_CTL_MAX_HEADER,
 * n > 2^40, tcp_ttl outside 1..255, an interface aipstack_icmp_rx_respond rejects, d_ctl,
 * d_chunk_index, d_counts or d_workspace not 8-byte aligned, d_hdr_len not 4-byte aligned, or
 * workspace_bytes < aipstack_tcp_tx_control_workspace_bytes(n). n == 0 is a no-op. */
#define AIPSTACK_TCP_CTL_MAX_HEADER 62u  /* 54 + MSS 4 + window scale 4 */
#define AIPSTACK_TCP_CTL_EMITTED  48     /* per descriptor: the slot holds its segment */
#define AIPSTACK_TCP_CTL_INVALID  49     /* per descriptor: a reserved field or an unknown option bit */

typedef struct aipstack_tcp_ctl {   /* 32 bytes, 8-byte aligned, host-made */
    uint32_t local_addr, remote_addr;   /* TcpPcbKey, host order as in aipstack_tcp_pcb_key */
    uint16_t local_port, remote_port;
    uint32_t seq, ack;                  /* stored as given (ack also where ACK is clear) */
    uint16_t window;                    /* stored as given (send_rst passes 0) */
    uint16_t mss;                       /* the MSS option's value */
    uint8_t  flags;                     /* low byte of OffsetFlags: FIN 01 SYN 02 RST 04 PSH 08 ACK 10 URG 20 ECE 40 CWR 80 */
    uint8_t  options;                   /* AIPSTACK_TCP_OPT_MSS | AIPSTACK_TCP_OPT_WND_SCALE */
    uint8_t  wnd_scale;
    uint8_t  reserved0;                 /* 0 */
    uint32_t reserved1;                 /* 0 */
} aipstack_tcp_ctl;

uint64_t aipstack_tcp_tx_control_workspace_bytes(uint64_t n);
int aipstack_tcp_tx_control(const aipstack_tcp_ctl *d_ctl, uint64_t n,
                            const aipstack_icmp_iface *h_iface, uint32_t tcp_ttl,
                            void *d_hdr, uint64_t hdr_stride, uint32_t *d_hdr_len,
                            uint64_t *d_chunk_index, uint8_t *d_status, uint64_t *d_counts,
                            void *d_workspace, uint64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AIPSTACK_AMD_CHKSUM_H */
