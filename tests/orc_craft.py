"""Hand-built ORC tails for corrupt-file tests: a minimal protobuf wire
writer for the PostScript / Footer / StripeInformation / Type messages
(field numbers from the ORC spec, site/specification/ORCv1.md "File Tail"),
so tests can produce offsets and lengths no writer would emit."""


def varint(x):
    out = bytearray()
    x &= (1 << 64) - 1
    while True:
        b = x & 0x7F
        x >>= 7
        if x:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def field_varint(f, v):
    return varint(f << 3) + varint(v)


def field_bytes(f, b):
    return varint((f << 3) | 2) + varint(len(b)) + b


def stripe_info(offset, index_length, data_length, footer_length, num_rows):
    return (field_varint(1, offset) + field_varint(2, index_length) + field_varint(3, data_length) +
            field_varint(4, footer_length) + field_varint(5, num_rows))


def type_msg(kind, subtypes=(), names=()):
    m = field_varint(1, kind)
    if subtypes:
        m += field_bytes(2, b"".join(varint(s) for s in subtypes))
    for n in names:
        m += field_bytes(3, n.encode())
    return m


def decimal_type(precision, scale):
    """Type{kind = DECIMAL, precision = 5, scale = 6} (precision 0: Hive 0.11)."""
    return type_msg(T_DECIMAL) + field_varint(5, precision) + field_varint(6, scale)


def orc_file(body, stripes, types, num_rows, footer_length_override=None, row_index_stride=None):
    """'ORC' + body + Footer + PostScript + 1-byte PostScript length
    (uncompressed). row_index_stride: Footer.rowIndexStride (field 8), left
    out when None."""
    footer = b"".join(field_bytes(3, s) for s in stripes)
    footer += b"".join(field_bytes(4, t) for t in types)
    footer += field_varint(6, num_rows)
    if row_index_stride is not None:
        footer += field_varint(8, row_index_stride)
    flen = len(footer) if footer_length_override is None else footer_length_override
    ps = field_varint(1, flen) + field_varint(2, 0) + field_bytes(4, varint(0) + varint(12)) + field_bytes(8000, b"ORC")
    return b"ORC" + body + footer + ps + bytes([len(ps)])


# ---- whole files: an uncompressed struct of non-nullable columns ------------
# Stream.Kind, ColumnEncoding.Kind and Type.Kind numbers (ORCv1.md "Stripe
# Footer", "Type Information")
PRESENT, DATA, LENGTH, DICTIONARY_DATA, SECONDARY, ROW_INDEX = 0, 1, 2, 3, 5, 6
ENC_DIRECT, ENC_DICTIONARY, ENC_DIRECT_V2, ENC_DICTIONARY_V2 = 0, 1, 2, 3
T_BOOLEAN, T_BYTE, T_SHORT, T_INT, T_LONG, T_STRING, T_STRUCT, T_DECIMAL = 0, 1, 2, 3, 4, 7, 12, 14


def stream_msg(kind, column, length):
    return field_varint(1, kind) + field_varint(2, column) + field_varint(3, length)


def encoding_msg(kind, dictionary_size=None):
    return field_varint(1, kind) + (b"" if dictionary_size is None else field_varint(2, dictionary_size))


def bool_rle(bits):
    """A PRESENT stream: bits MSB first into bytes, byte RLE as literal groups
    of at most 128 bytes (ORCv1.md "Boolean Run Length Encoding")."""
    padded = list(bits) + [0] * (-len(bits) % 8)
    by = bytes(sum(int(b) << (7 - j) for j, b in enumerate(padded[i:i + 8])) for i in range(0, len(padded), 8))
    out = bytearray()
    for i in range(0, len(by), 128):
        chunk = by[i:i + 128]
        out.append(256 - len(chunk))
        out += chunk
    return bytes(out)


def row_index_msg(entries):
    """RowIndex{ repeated RowIndexEntry entry = 1 { repeated uint64 positions
    = 1 [packed] } }: entries = one list of positions per row group (an empty
    list gives an entry without positions, as the root struct has)."""
    out = b""
    for e in entries:
        out += field_bytes(1, field_bytes(1, b"".join(varint(p) for p in e)) if len(e) else b"")
    return out


class CraftColumn:
    """One column of one stripe: its streams [(Stream.Kind, bytes)] in file
    order, its ColumnEncoding, and (for a row index) its positions, one list
    per row group in the order the readers consume them (ORCv1.md "Indexes":
    uncompressed integer stream: byte offset of the run, values to skip in
    it; a dictionary string column: the pair of DATA; a direct string column:
    the DATA byte offset, then the pair of LENGTH)."""

    def __init__(self, streams, positions=None, encoding=ENC_DIRECT_V2, dictionary_size=None):
        self.streams = [(k, bytes(b)) for k, b in streams]
        self.positions = positions
        self.encoding = encoding
        self.dictionary_size = dictionary_size


def struct_stripe(columns, row_index=True):
    """(index section, data section, stripe footer) of a stripe whose root
    struct (column 0, no streams, DIRECT) has `columns` (CraftColumn, ids 1..)
    as children, none with a PRESENT stream. With row_index, the index section
    holds one ROW_INDEX stream per column, the root's with empty entries."""
    index, data, sf = b"", b"", b""
    if row_index:
        groups = len(columns[0].positions)
        for cid, c in enumerate([None] + list(columns)):
            entries = [[]] * groups if c is None else [[int(p) for p in e] for e in c.positions]
            assert len(entries) == groups
            m = row_index_msg(entries)
            index += m
            sf += field_bytes(1, stream_msg(ROW_INDEX, cid, len(m)))
    for cid, c in enumerate(columns, start=1):
        for kind, b in c.streams:
            data += b
            sf += field_bytes(1, stream_msg(kind, cid, len(b)))
    sf += field_bytes(2, encoding_msg(ENC_DIRECT))
    for c in columns:
        sf += field_bytes(2, encoding_msg(c.encoding, c.dictionary_size))
    return index, data, sf


def struct_file(names, kinds, stripes, row_index_stride):
    """An uncompressed file of struct<names[i]: kinds[i]> (Type.Kind numbers,
    or whole Type messages as bytes: decimal_type) with any number of stripes
    = [(num_rows, [CraftColumn per column])]. A row_index_stride of 0 writes
    no index section."""
    body, infos, total = b"", [], 0
    for num_rows, columns in stripes:
        assert len(columns) == len(names)
        index, data, sf = struct_stripe(columns, row_index=row_index_stride > 0)
        infos.append(stripe_info(3 + len(body), len(index), len(data), len(sf), num_rows))
        body += index + data + sf
        total += num_rows
    types = [type_msg(T_STRUCT, list(range(1, len(names) + 1)), names)]
    types += [k if isinstance(k, bytes) else type_msg(k) for k in kinds]
    return orc_file(body, infos, types, total, row_index_stride=row_index_stride)


# ---- whole files: an arbitrary type tree ------------------------------------------
T_LIST, T_MAP, T_UNION = 10, 11, 13


def tree_stripe(columns, groups):
    """(index section, data section, stripe footer) of a stripe whose columns
    (CraftColumn per type id, the root first; any may carry a PRESENT stream
    among its streams) are written in type-id order. groups: the row groups of
    the row index (0: no index section); a column's positions hold one list
    per row group (None: entries without positions, as a struct without a
    PRESENT stream has), in the order the readers consume them: PRESENT's
    byte offset, bytes to skip and bits to skip, then the kind's streams."""
    index, data, sf = b"", b"", b""
    if groups:
        for cid, c in enumerate(columns):
            entries = [[]] * groups if c.positions is None else [[int(p) for p in e] for e in c.positions]
            assert len(entries) == groups, (cid, len(entries), groups)
            m = row_index_msg(entries)
            index += m
            sf += field_bytes(1, stream_msg(ROW_INDEX, cid, len(m)))
    for cid, c in enumerate(columns):
        for kind, b in c.streams:
            data += b
            sf += field_bytes(1, stream_msg(kind, cid, len(b)))
    for c in columns:
        sf += field_bytes(2, encoding_msg(c.encoding, c.dictionary_size))
    return index, data, sf


def tree_file(types, stripes, row_index_stride):
    """An uncompressed file of the type tree `types` (Type messages in type-id
    order, type_msg) with stripes = [(num_rows, [CraftColumn per type id])];
    the row groups are row_index_stride top-level rows each (0: no index)."""
    body, infos, total = b"", [], 0
    for num_rows, columns in stripes:
        assert len(columns) == len(types)
        groups = (num_rows + row_index_stride - 1) // row_index_stride if row_index_stride else 0
        index, data, sf = tree_stripe(columns, groups)
        infos.append(stripe_info(3 + len(body), len(index), len(data), len(sf), num_rows))
        body += index + data + sf
        total += num_rows
    return orc_file(body, infos, types, total, row_index_stride=row_index_stride)
