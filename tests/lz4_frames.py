"""A strict walker over LZ4 frames: plain Python, runs no decoder.

walk(frame, plain_len) -> [(stored, n_plain, n_comp, [(ll, ml, off), ...]), ...], one tuple per block; the sequence list of a stored block
is empty, the last sequence of a compressed block is (ll, 0, 0).  Any violation raises AssertionError whose text names the rule (one of
RULES) and the block.  The rules are those of the LZ4 frame and block formats plus the encoder's own: a block goes out compressed only
when that makes it strictly smaller (lz4e_write_block: limit = n - 1; liblz4's LZ4F_makeBlock does the same), and the end-of-block
rules no decoder here checks: the last 5 bytes of a block are literals and its last match starts at least 12 bytes before its end."""
import struct

from tests._libs import oracle

MAGIC = 0x184D2204
BLOCK_MAX = {4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}
MFLIMIT, LASTLIT, MINMATCH = 12, 5, 4
RULES = ("magic", "FLG version", "FLG reserved", "BD reserved", "BD block size", "header truncated", "HC", "content size",
         "EndMark", "block size word", "block truncated", "stored size", "short block compressed", "compressed not smaller",
         "block checksum", "content checksum", "length extension", "block end", "offset zero", "offset beyond history", "match length",
         "last literals", "last match start", "trailing bytes", "plain length", "block not full")


def _need(cond, rule, block, detail=""):
    assert rule in RULES
    if not cond:
        raise AssertionError("LZ4 frame rule '%s' violated in block %s: %s" % (rule, block, detail))


def _length(data, p, end, nibble, b):
    """a length whose token nibble is `nibble`: -> (value, position behind its extension bytes)"""
    v = nibble
    if nibble == 15:
        while True:
            _need(p < end, "length extension", b, "a run of 255s reaches the block's end")
            x = data[p]
            p += 1
            v += x
            if x < 255:                                      # (a run ends in a byte below 255: the one encoding of the value)
                break
    return v, p


def _sequences(data, at, n_comp, produced, linked, b):
    """the sequences of the compressed block data[at, at + n_comp); `produced` plain bytes lie before it in the frame"""
    p, end, out, seqs = at, at + n_comp, 0, []
    last_match_start = None
    while True:
        _need(p < end, "block end", b, "the block ends behind a match, not in a literals-only sequence")
        tok = data[p]
        ll, p = _length(data, p + 1, end, tok >> 4, b)
        _need(p + ll <= end, "block end", b, "%d literals at byte %d of %d" % (ll, p - at, n_comp))
        p += ll
        out += ll
        if p == end:
            _need(tok & 15 == 0, "block end", b, "the last token carries a match length")
            seqs.append((ll, 0, 0))
            break
        _need(p + 2 <= end, "block end", b, "half an offset")
        off = data[p] | (data[p + 1] << 8)
        ml, p = _length(data, p + 2, end, tok & 15, b)
        ml += MINMATCH
        _need(off >= 1, "offset zero", b, "sequence %d" % len(seqs))
        history = min(65535, (produced if linked else 0) + out)
        _need(off <= history, "offset beyond history", b, "sequence %d: offset %d, %d bytes to go back over" % (len(seqs), off, history))
        _need(ml >= MINMATCH, "match length", b, ml)
        last_match_start = out
        out += ml
        seqs.append((ll, ml, off))
    return out, seqs, last_match_start


def walk(frame, plain_len):
    data = bytes(frame)
    size = len(data)
    o = oracle()
    _need(size >= 7, "header truncated", "-", size)
    _need(struct.unpack_from("<I", data, 0)[0] == MAGIC, "magic", "-", data[:4].hex())
    flg, bd = data[4], data[5]
    _need(flg >> 6 == 1, "FLG version", "-", flg >> 6)
    _need(flg & 0x02 == 0, "FLG reserved", "-", hex(flg))
    _need(bd & 0x8F == 0, "BD reserved", "-", hex(bd))
    _need((bd >> 4) & 7 in BLOCK_MAX, "BD block size", "-", (bd >> 4) & 7)
    block_max = BLOCK_MAX[(bd >> 4) & 7]
    linked, block_sum, has_size, content_sum, has_dict = not flg & 0x20, bool(flg & 0x10), bool(flg & 0x08), bool(flg & 0x04), bool(flg & 0x01)
    p = 6 + (8 if has_size else 0) + (4 if has_dict else 0)
    _need(p + 1 <= size, "header truncated", "-", size)
    _need(data[p] == (o.xxh32(data[4:p]) >> 8) & 0xFF, "HC", "-", "%#x, the descriptor's is %#x" % (data[p], (o.xxh32(data[4:p]) >> 8) & 0xFF))
    if has_size:
        _need(struct.unpack_from("<Q", data, 6)[0] == plain_len, "content size", "-", struct.unpack_from("<Q", data, 6)[0])
    p += 1
    blocks, produced = [], 0
    while True:
        b = len(blocks)
        _need(p + 4 <= size, "EndMark", b, "the frame ends without one")
        word = struct.unpack_from("<I", data, p)[0]
        p += 4
        if word == 0:
            break
        stored, n_comp = bool(word >> 31), word & 0x7FFFFFFF
        _need(n_comp <= block_max, "block size word", b, n_comp)
        _need(p + n_comp + (4 if block_sum else 0) <= size, "block truncated", b, "%d bytes, %d left" % (n_comp, size - p))
        if stored:
            _need(n_comp <= plain_len - produced, "stored size", b, "%d bytes stored, %d of the plaintext left" % (n_comp, plain_len - produced))
            n_plain, seqs = n_comp, []
        else:
            n_plain, seqs, last_match_start = _sequences(data, p, n_comp, produced, linked, b)
            _need(n_plain > MFLIMIT, "short block compressed", b, "%d plain bytes" % n_plain)
            _need(seqs[-1][0] >= LASTLIT, "last literals", b, "%d literals behind the last match" % seqs[-1][0])
            if last_match_start is not None:
                _need(n_plain - last_match_start >= MFLIMIT, "last match start", b, "it starts %d bytes before the block's end" % (n_plain - last_match_start))
            _need(n_comp < n_plain, "compressed not smaller", b, "%d bytes for %d" % (n_comp, n_plain))
            _need(n_plain <= block_max, "block size word", b, "%d plain bytes" % n_plain)
        if block_sum:
            _need(struct.unpack_from("<I", data, p + n_comp)[0] == o.xxh32(data[p:p + n_comp]), "block checksum", b)
        p += n_comp + (4 if block_sum else 0)
        produced += n_plain
        blocks.append((stored, n_plain, n_comp, seqs))
    # (the checksum is that of the plaintext, which a walker that runs no decoder does not have: its four bytes must be there)
    _need(size - p >= (4 if content_sum else 0), "content checksum", "-", "missing")
    _need(size - p == (4 if content_sum else 0), "trailing bytes", "-", "%d bytes behind the frame's end" % (size - p - (4 if content_sum else 0)))
    _need(produced == plain_len, "plain length", "-", "%d bytes in the blocks, %d expected" % (produced, plain_len))
    for b, blk in enumerate(blocks[:-1]):
        _need(blk[1] == block_max, "block not full", b, blk[1])
    return blocks
