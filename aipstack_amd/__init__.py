"""aipstack_amd -- MI355X-native Internet-checksum engine for aipstack's packet path.

The product is ``aipstack_amd/lib/libaipstack_chksum.so`` (host C++ + CDNA4 HIP
kernels) behind the C-ABI in ``include/aipstack_amd/chksum.h``; this package is its
Python host-side mirror (``chksum``) plus synthetic-batch plumbing (``synth``).
Importing it loads the native library and fails loudly if it was not built.
"""
from . import _lib

_lib.load()

from . import chksum  # noqa: E402

LIB_PATH = _lib.LIB_PATH

# The public names, all of them chksum's (the engine classes through its re-import of
# engine.py): the one list behind both the package's attributes and __all__.
_FROM_CHKSUM = [
    "AIPSTACK_CHKSUM_EHIP",
    "AIPSTACK_CHKSUM_EINVAL",
    "AIPSTACK_CHKSUM_ENODEV",
    "AIPSTACK_CHKSUM_FINAL",
    "AIPSTACK_CHKSUM_JUST_WRITTEN",
    "AIPSTACK_CHKSUM_MAX_LEN",
    "AIPSTACK_CHKSUM_OK",
    "ChksumEngine",
    "ChksumEngineGroup",
    "ChksumError",
    "IpBufNode",
    "IpBufRef",
    "IpChksum",
    "IpChksumAccumulator",
    "IpChksumInverted",
    "chksum_batch_chain",
    "chksum_chain_fill",
    "chksum_batch_csr",
    "chksum_batch_seeded_csr",
    "chksum_batch_slotted",
    "chksum_batch_strided",
    "contract_violations",
    "device_check",
    "VIOLATION_CHUNK_LEN",
    "VIOLATION_PACKET_LEN",
    "VIOLATION_SPAN",
    "flatten_chains",
    "ipBufProcessBytes",
    "RX_VERDICTS",
    "rx_verify",
    "rx_verify_slotted",
    "slots_to_offsets",
    "tx_fill",
    "tx_fill_records",
    "tx_fill_records_slotted",
    "tx_fill_slotted",
    "apply_tx_records",
    "AIPSTACK_CHKSUM_MAX_SPLIT_HEADER",
    "AIPSTACK_TX_SPLIT_LAYOUT",
    "SplitFrames",
    "split_frames",
    "tx_fill_header_split",
    "AIPSTACK_TCP_BURST_FIN",
    "AIPSTACK_TCP_SEGMENT_HEADER",
    "AIPSTACK_TX_BURST_INVALID",
    "TCP_BURST_DTYPE",
    "TcpSegments",
    "tcp_burst_layout",
    "tcp_tx_segment",
    "AIPSTACK_TX_DGRAM_INVALID",
    "AIPSTACK_TX_FRAG_NEEDED",
    "AIPSTACK_UDP_FIRST_FRAGMENT_HEADER",
    "AIPSTACK_UDP_MIN_MTU",
    "AIPSTACK_UDP_NEXT_FRAGMENT_HEADER",
    "UDP_DGRAM_DTYPE",
    "UdpFragments",
    "udp_dgram_layout",
    "udp_tx_fragment",
    "AIPSTACK_RX_DROP_TCP_OFFSET",
    "AIPSTACK_TCP_NO_PCB",
    "AIPSTACK_TCP_OPT_MSS",
    "AIPSTACK_TCP_OPT_WND_SCALE",
    "AIPSTACK_TCP_SEG_VALID",
    "TCP_PCB_KEY_DTYPE",
    "TCP_RX_SEG_DTYPE",
    "TcpRxParsed",
    "tcp_pcb_table_sort",
    "tcp_rx_parse",
    "tcp_rx_parse_slotted",
    "AIPSTACK_IP4_MAX_REASS_SIZE",
    "AIPSTACK_REASS_NONE",
    "AIPSTACK_RX_DROP_FRAG",
    "AIPSTACK_RX_FRAG_MEMBER",
    "AIPSTACK_RX_REASS_TRUNCATED",
    "IP4_DGRAM_DTYPE",
    "Ip4Reassembled",
    "ip4_reass_workspace_bytes",
    "ip4_rx_reassemble",
    "ip4_rx_reassemble_slotted",
    "AIPSTACK_CHKSUM_MAX_SLOT_STRIDE",
    "AIPSTACK_TX_LIN_INVALID",
    "AIPSTACK_TX_LIN_SKIPPED",
    "AIPSTACK_TX_LIN_TOO_LARGE",
    "AIPSTACK_TX_LIN_TOO_SHORT",
    "AIPSTACK_TX_LIN_WRITTEN",
    "AIPSTACK_TX_LIN_WRONG_ROOM",
    "LinearFrames",
    "tx_linearise",
    "tx_linearise_slotted",
]
globals().update((name, getattr(chksum, name)) for name in _FROM_CHKSUM)

__all__ = _FROM_CHKSUM + ["LIB_PATH"]
