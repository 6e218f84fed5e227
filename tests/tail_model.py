"""in_tail's line packing restated in plain Python, and a model of which path of k_tl_emit a text reaches.

records() follows plugins/in_tail/tail_file.c's plain path (process_content :689-1040 + flb_tail_file_pack_line :552-604) by its
rules, as oracle/oflb.c oflb_tail_process restates them, without calling the oracle: leading NULs are consumed, the text is cut at
'\\n', an empty line or a lone '\\r' is skipped under Skip_Empty_Lines, a line of two bytes or more loses one trailing '\\r', and
every kept line becomes  92 92 d7 00 <sec> <nsec> | df 00 00 00 00 | df 00 00 00 nn | [path_key path] [offset_key uint] key line
with msgpack's smallest encodings.  It returns one row per newline (b"" for a skipped line): the row table of the device chunk.

emit_paths() mirrors only the batching decision of k_tl_emit (csrc/tail_kernels.inc), from the records' sizes alone.  The tests use
it to assert that a text reaches the path it was written for; it computes no bytes.  Its constants are compared with the .inc's."""
import struct

TL_TILE = 16384           # bytes per workgroup of k_tl_count / k_tl_fill
TL_TILE_T = 256           # its threads, 64 bytes each
TL_STG = 18944            # staging bytes per wave of k_tl_emit
SIZE_BLOCKS = 4096        # k_tl_size: at most this many workgroups of 256 lanes
EMIT_BLOCKS_PER_CU = 8    # k_tl_emit: at most cus * 8 workgroups of 4 waves, 64 rows per wave and trip


def pack_str(b):
    n = len(b)
    if n < 32:
        return bytes([0xa0 | n]) + b
    if n < 256:
        return bytes([0xd9, n]) + b
    if n < 65536:
        return b"\xda" + struct.pack(">H", n) + b
    return b"\xdb" + struct.pack(">I", n) + b


def pack_uint(v):
    if v < 128:
        return bytes([v])
    if v < 256:
        return bytes([0xcc, v])
    if v < 65536:
        return b"\xcd" + struct.pack(">H", v)
    if v < 1 << 32:
        return b"\xce" + struct.pack(">I", v)
    return b"\xcf" + struct.pack(">Q", v)


def _b(x):
    return x if isinstance(x, bytes) else x.encode()


def records(text, key="log", path_key=None, path="", offset_key=None, stream_offset=0, skip_empty_lines=True, sec=0, nsec=0):
    """-> (rows, processed): rows[i] is the record of the line that newline i ends, or b"" where the reference skips the line"""
    lead = 0
    while lead < len(text) and text[lead] == 0:
        lead += 1
    lines = text[lead:].split(b"\n")
    lines.pop()                                       # what follows the last newline stays in the file's buffer
    if not lines:
        return [], lead
    nbody = 1 + (1 if path_key else 0) + (1 if offset_key else 0)
    head = b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + b"\xdf\0\0\0\0" + b"\xdf\0\0\0" + bytes([nbody])
    if path_key:
        head += pack_str(_b(path_key)) + pack_str(_b(path or ""))
    okey = pack_str(_b(offset_key)) if offset_key else None
    kkey = pack_str(_b(key or "log"))
    rows, pos = [], lead
    for line in lines:
        n = len(line)
        if skip_empty_lines and (n == 0 or line == b"\r"):
            rows.append(b"")
        else:
            if n >= 2 and line[-1] == 13:
                line = line[:-1]
            if okey is None:
                rows.append(head + kkey + pack_str(line))
            else:
                rows.append(head + okey + pack_uint(stream_offset + pos) + kkey + pack_str(line))
        pos += n + 1
    return rows, pos


def second_trips(nl, cus):
    """(k_tl_size, k_tl_emit): whether a text of nl newlines sends a lane / a wave round its grid-stride loop again"""
    tiles = (nl + 63) // 64
    blocks = min((tiles + 3) // 4, cus * EMIT_BLOCKS_PER_CU)
    return nl > SIZE_BLOCKS * 256, tiles > blocks * 4


def emit_paths(row_sizes, stg=TL_STG, cus=256):
    """the batching decision of k_tl_emit over tiles of 64 rows: a batch runs from row `lo` of the tile over the rows that end within
    `stg` bytes of the batch's first byte rounded down to 16; a row that does not fit even alone (m == 0) goes straight to global
    memory.  -> dict(direct=[(tile, lane)], exact=[(tile, lane, align)], batches=[per tile], aligns={...}, size_trip2, emit_trip2)"""
    n = len(row_sizes)
    off = [0] * (n + 1)
    for i, s in enumerate(row_sizes):
        off[i + 1] = off[i] + s
    direct, exact, batches, aligns = [], [], [], set()
    for t in range((n + 63) // 64):
        base, cnt = t * 64, min(64, n - t * 64)
        lo = nb = 0
        while lo < cnt:
            bb = off[base + lo]
            align = bb & 15
            m = 0
            while lo + m < cnt and off[base + lo + m + 1] - bb + align <= stg:
                m += 1
            if m == 0:
                direct.append((t, lo))
                lo += 1
                continue
            total = off[base + lo + m] - bb
            if total:
                nb += 1
                aligns.add(align)
                if total + align == stg:
                    exact.append((t, lo, align))
            lo += m
        batches.append(nb)
    t2 = second_trips(n, cus)
    return dict(direct=direct, exact=exact, batches=batches, aligns=aligns, size_trip2=t2[0], emit_trip2=t2[1])
