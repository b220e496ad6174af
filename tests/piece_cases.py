"""The cases of the piece-copy and text kernels run on the host
(tests/test_piece_host_cpu.py) and, the gather's valid ones, on the GPU
(tests/test_piece_cases_gpu.py).  Not a test module: pure functions that
return lists of cases, no device and no subprocess.  A case is a dict; what is
not a number, a list of numbers or bytes in it (the keys that start with "_")
is for the test's own reference and is not sent to the program.

Every text here is handed to the program as it is: the program gives it an
allocation of exactly its length, so a text's last byte is the last byte of
its allocation by construction, in every case -- no case needs a variant of its
own for that."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_rule as R  # noqa: E402

U32, U64 = 1 << 32, 1 << 64
PAGE = 4096
LENGTHS = (0, 1, 8, 15, 16, 17, 33)


def image_byte(i: int) -> int:
    """Byte i of the host program's image."""
    return (i * 131 + 7) & 0xFF


def image_bytes_at(pos: int, n: int, image_bytes: int) -> bytes:
    """n bytes from `pos` of the host program's image; bytes at or past its end read as 0."""
    return bytes(image_byte(p) if p < image_bytes else 0 for p in range(pos, pos + n))


# ---- gather: valid scans -------------------------------------------------------------------------------------

def place(vlens, scale=1, image_bytes=None):
    """Sources for values of these lengths such that consecutive values are not adjacent in the image, the first
    value farthest in.  Without `image_bytes` the image ends with the last byte of the value that reaches
    farthest: (src, image_bytes).  With it (an image that exists already), every value lies inside it."""
    n = len(vlens)
    step = 61 if scale == 1 else 5
    assert n == 1 or max(vlens) < step * scale
    if image_bytes is None and n <= 100:
        src = [2 + (n - 1 - i) * step for i in range(n)]
        return src, max(s * scale + l for s, l in zip(src, vlens))
    if image_bytes is None:
        image_bytes = 4099
    span = (image_bytes - max(vlens)) // scale + 1          # sources 0 .. span - 1 keep every value inside
    assert n == 1 or span > 2 * step
    return [((n - 1 - i) * step + 2) % span for i in range(n)], image_bytes


def gather_case(vlens, mis, scale=1, cus=256):
    voff = [0]
    for l in vlens:
        voff.append(voff[-1] + l)
    src, image_bytes = place(vlens, scale)
    return dict(mode="gather", mis=mis, scale=scale, cus=cus, image_bytes=image_bytes, voff=voff, src=src,
                value_bytes=voff[-1], _vlens=list(vlens))


def sequences(lengths):
    out = [(a,) for a in lengths]
    out += [(a, b) for a in lengths for b in lengths]
    out += [(a, b, c) for a in lengths for b in lengths for c in lengths]
    return [s for s in out if sum(s)]                        # (an output of 0 bytes is no launch)


def scan_of(total, each=3):
    """Values of `each` bytes, and a shorter last one, that make `total` bytes."""
    return [each] * (total // each) + ([total % each] if total % each else [])


def gather_enumeration():
    """Every misalignment x every sequence of one, two or three lengths of LENGTHS."""
    return [gather_case(s, mis) for mis in range(16) for s in sequences(LENGTHS)]


def gather_enumeration_scale8():
    """The same with 8-byte slots as sources (approximate mode): lengths cut to 8, four misalignments."""
    cut = sorted({min(l, 8) for l in LENGTHS})
    return [gather_case(s, mis, scale=8) for mis in (0, 1, 8, 15) for s in sequences(cut)]


def gather_edges():
    """64 pieces are a wave, 256 a workgroup: totals around 1024 and 4096 bytes, as 3-byte values and as one."""
    out = []
    for mis in (0, 5, 15):
        for total in (1023, 1024, 1025, 4095, 4096, 4097):
            out += [gather_case(scan_of(total), mis), gather_case([total], mis)]
    return out


def gather_second_trip():
    """One CU: the grid is capped at 32 workgroups = 8192 pieces, so 131 072 + 17 bytes need a second trip of
    the loop, whose only wave is partial."""
    total = 131072 + 17
    out = []
    for mis in (0, 5, 15):
        out += [gather_case(scan_of(total), mis, cus=1), gather_case([total], mis, cus=1)]
    return out


def gather_empty_runs():
    out = []
    for mis in (0, 5, 15):
        out.append(gather_case([1] + [0] * 70 + [1], mis))   # the owner search steps over more than a wave of entries
        out.append(gather_case([0, 0, 5, 0, 17, 0, 0], mis))  # starts and ends with empty values
        out.append(gather_case([1] * 40, mis))               # many sources in one piece
    return out


def gather_valid_gpu():
    """What runs on the GPU too: the enumeration at scale 1, the wave / workgroup edges, the empty runs."""
    return gather_enumeration() + gather_edges() + gather_empty_runs()


def gather_valid():
    return gather_valid_gpu() + gather_enumeration_scale8() + gather_second_trip()


# ---- gather: offsets that are no scan, sources anywhere ------------------------------------------------------

def gather_hostile(seed=5, per_family=14):
    """Seeded; image_bytes 1 .. 300, scale 1 and 8.  `_family` names what was done to a valid case."""
    rng = np.random.default_rng(seed)

    def word():
        return int(rng.integers(0, U64, dtype=np.uint64))

    out = []
    for family in ("random", "below_total", "every_second", "decreasing", "tail_zeros", "tail_ones", "src"):
        for j in range(per_family):
            n = int(rng.integers(1, 41))
            vlens = [int(x) for x in rng.integers(0, 20, n)]
            if not sum(vlens):
                vlens[0] = 3
            scale = (1, 8)[j % 2]
            image_bytes = int(rng.integers(1, 301))
            voff = [0]
            for l in vlens:
                voff.append(voff[-1] + l)
            total = voff[-1]
            src = [int(rng.integers(0, max(1, image_bytes // scale))) for _ in range(n)]
            if family == "random":
                voff = [word() for _ in voff]
            elif family == "below_total":
                voff = [int(x) for x in rng.integers(0, total + 5, n + 1)]
            elif family == "every_second":
                voff = [v if i % 2 == 0 else U64 - 1 - int(rng.integers(0, 1000)) for i, v in enumerate(voff)]
            elif family == "decreasing":
                voff = voff[::-1]
            elif family in ("tail_zeros", "tail_ones"):
                cut = int(rng.integers(1, n + 1))
                voff = voff[:cut] + [0 if family == "tail_zeros" else U64 - 1] * (n + 1 - cut)
            else:
                near = [image_bytes + d for d in range(-8, 9) if image_bytes + d >= 0]
                src = [(word(), U64 - 1, near[int(rng.integers(0, len(near)))], s)[int(rng.integers(0, 4))] for s in src]
            out.append(dict(mode="gather", mis=int(rng.integers(0, 16)), scale=scale, cus=256, image_bytes=image_bytes,
                            voff=voff, src=src, value_bytes=total, _family=family))
    return out


def gather_promised(case):
    """What a gather over any offsets still owes: [(output byte, its value)] for every byte that a valid prefix
    of the offsets covers.  The prefix [0, k] is valid when voff[0] = 0, voff[0 .. k] does not decrease and no
    later word is below voff[k]: then `voff[i] <= o` is true up to the owner of o and false after it for every
    o < voff[k], which is all a binary search needs, whatever the later words are.  A byte's value is the image
    byte at src * scale + its offset in the value, 0 at or past the image's end (the bounded reader's rule).  A
    value whose positions pass 2^64 owes nothing: the kernel's position arithmetic is modulo 2^64 and it reads
    8 source bytes a step, so which of the wrapped positions read as "past the end" depends on where a piece
    starts.  Everything else may be anything."""
    voff, src = case["voff"], case["src"]
    if voff[0] != 0:
        return []
    k = 0
    while k + 1 < len(voff) and voff[k + 1] >= voff[k]:
        k += 1
    while k and any(w < voff[k] for w in voff[k + 1:]):
        k -= 1
    out = []
    for q in range(k):
        if src[q] * case["scale"] + (voff[q + 1] - voff[q]) + 8 >= U64:
            continue
        for o in range(voff[q], min(voff[q + 1], case["value_bytes"])):
            p = src[q] * case["scale"] + (o - voff[q])
            out.append((o, image_byte(p) if p < case["image_bytes"] else 0))
    return out


# ---- pack and pack_blocked -----------------------------------------------------------------------------------

def pack_case(recs, mis, parts=1, B=0, before=None, terminate_last=True, name=""):
    """recs: [(key, value)].  The text is the records as "key value\\n" lines (the last one without its
    terminator when terminate_last is false: its value ends the text), the descriptors point into it.  image_cap
    and blob_cap are the caller's buffers (the library refuses sizes that pass them): what the largest records
    would need, whatever the descriptors say."""
    text, desc, pos = bytearray(), [], 0
    for i, (k, v) in enumerate(recs):
        line = k + b" " + v + (b"\n" if terminate_last or i + 1 < len(recs) else b"")
        desc.append((pos, len(k), pos + len(k) + 1, len(v)))
        text += line
        pos += len(line)
    kpos, klen, vpos, vlen = (list(x) for x in zip(*desc))
    c = dict(mode="pack_blocked" if B else "pack", mis=mis, parts=parts, text=bytes(text), kpos=kpos, klen=klen, vpos=vpos,
             vlen=vlen, before=list(before) if before else ([0] * parts if B else [1000 * p + 7 for p in range(parts)]),
             image_cap=2 * (3 + R.MAX_KEY + R.MAX_VALUE) * len(recs) + parts * B + 16, blob_cap=R.MAX_KEY * len(recs), _name=name)
    if B:
        c["B"] = B
    return c


def described_records(case):
    """The records a pack owes for any descriptors: lengths cut to 255 and 32 510 (text_klen / text_vlen), bytes
    whose source lies at or past the text's end 0."""
    text = case["text"]

    def fetch(pos, n):
        return text[pos:pos + n].ljust(n, b"\0")

    return [(fetch(kp, min(kl, R.MAX_KEY)), fetch(vp, min(vl, R.MAX_VALUE)))
            for kp, kl, vp, vl in zip(case["kpos"], case["klen"], case["vpos"], case["vlen"])]


SHORT3 = [(b"a", b"b"), (b"cd", b"e"), (b"f", b"gh")]     # test_pack_short_destinations_at_every_misalignment's


def _value(n, i=0):
    return ((np.arange(n, dtype=np.uint32) * 7 + i) % 26 + 0x41).astype(np.uint8).tobytes()


def _some_records(n, seed):
    rng = np.random.default_rng(seed)
    return [(b"k%d" % i, _value(int(rng.integers(1, 30)), i)) for i in range(n)]


def pack_valid(B=0):
    out = []
    for mis in range(16):
        out += [pack_case(SHORT3[:1], mis, B=B, name="short1"), pack_case(SHORT3, mis, B=B, name="short3")]
    for vl in (256, 257, 32510):                             # from 256 on the header's second byte is not 0
        out.append(pack_case([(b"x", b"y"), (b"big", _value(vl)), (b"z", b"w")], 3, B=B, name=f"value{vl}"))
        out.append(pack_case([(b"big", _value(vl))], 9, B=B, name=f"value{vl}_alone"))
    out.append(pack_case([(b"x", b"y"), (b"K" * 255, b"v" * 5), (b"z", b"w")], 5, B=B, name="key255"))
    out.append(pack_case([(b"K" * 255, _value(32510))], 11, B=B, name="largest_record"))
    for recs in (SHORT3, [(b"key", _value(40))], [(b"x", b"y"), (b"big", _value(300))]):
        out.append(pack_case(recs, 7, B=B, terminate_last=False, name="value_ends_the_text"))
    recs = _some_records(20, 3)
    for parts in (1, 3, 8):
        out.append(pack_case(recs, 3, parts=parts, B=B, before=[PAGE * (p + 1) for p in range(parts)] if B else None,
                             name=f"parts{parts}"))
    out.append(pack_case(recs[:5], 13, parts=8, B=B, name="5_records_8_parts"))
    out.append(pack_case(recs[:2], 1, parts=3, B=B, name="2_records_3_parts"))
    return out


def blocked_table():
    """The rule table of tests/test_text_blocked_gpu.py as it is, and shapes that cross a 2 048-record tile."""
    import test_text_blocked_gpu as G
    out = []
    for i, name in enumerate(sorted(G.TABLE)):
        recs = [G.record(j, s) for j, s in enumerate(G.TABLE[name])]
        out.append(pack_case(recs, (3 * i) % 16, B=PAGE, name=name))
    for sizes, parts in (([5] * 4200, 1), ([5] * 4200, 3), ([9] * 2048 + [4000] + [9] * 100, 1)):
        recs = [G.record(j, s) for j, s in enumerate(sizes)]
        out.append(pack_case(recs, 3, parts=parts, B=PAGE, name=f"tiles_{len(sizes)}_{parts}"))
    return out


def pack_hostile(B=0, seed=9):
    """Four honest records, and one descriptor among them with lengths no record has or positions at and past the
    text's end; then all four words random."""
    rng = np.random.default_rng(seed)
    recs = [(b"alpha", b"one"), (b"beta", _value(25)), (b"gamma", b"3"), (b"delta", _value(9)), (b"eps", b"five")]
    base = pack_case(recs, 0, B=B)
    nbytes = len(base["text"])
    out = []

    def variant(changes, parts=1, name=""):
        c = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
        for (field, i), v in changes.items():
            c[field][i] = v
        c.update(mis=int(rng.integers(0, 16)), parts=parts, before=[0] * parts if B else [1000 * p + 7 for p in range(parts)],
                 _name=name)
        out.append(c)

    lens = (256, 32511, 65536, U32 - 1)
    poss = (nbytes - 1, nbytes, nbytes + 1, U32 - 1)
    for i, v in enumerate(lens):
        variant({("klen", i): v}, name=f"klen{v}")
        variant({("vlen", i): v}, name=f"vlen{v}")
        variant({("klen", i): v, ("vlen", i): lens[3 - i]}, parts=2, name=f"klen{v}_vlen{lens[3 - i]}")
    for i, v in enumerate(poss):
        variant({("kpos", i): v}, name=f"kpos{v}")
        variant({("vpos", i): v}, name=f"vpos{v}")
        variant({("kpos", i): v, ("klen", i): 300, ("vpos", i): poss[3 - i], ("vlen", i): 40000}, parts=3, name=f"pos{v}_long")
    variant({("vpos", 4): nbytes - 3, ("vlen", 4): 8}, name="value_head_crosses_the_end")
    for j in range(12):
        changes = {(f, i): int(rng.integers(0, U32)) for f in ("kpos", "klen", "vpos", "vlen") for i in range(5)
                   if j % 2 == 0 or i == j % 5}
        variant(changes, parts=1 + j % 3, name=f"random{j}")
    return out


# ---- split ---------------------------------------------------------------------------------------------------

def split_cases():
    import test_text_gpu as G
    mark = [m for m in G.test_degenerate_texts.pytestmark if m.name == "parametrize"][0]
    assert mark.args[0] == "text"
    out = [dict(mode="split", sep=32, text=t, _name="degenerate") for t in mark.args[1]]
    for o in G.EDGES:                                        # the texts of test_piece_and_block_edges
        out.append(dict(mode="split", sep=32, text=b"k " + b"v" * (o - 3) + b"\n" + b"x y\nz w", _name=f"line_start{o}"))
        out.append(dict(mode="split", sep=32, text=b"p " + b"q" * (o - 6) + b"\n" + b"abc val\r\nz w\n", _name=f"separator{o}"))
        out.append(dict(mode="split", sep=32, text=b"k " + b"v" * (o - 3) + b"\r\n" + b"x y\rz w\r\n", _name=f"crlf{o}"))
    for sep in (b" ", b"\t", b","):                          # the rule table, with and without its last terminator
        lines = [t.replace(" ", sep.decode()).encode() for t in G.TABLE] * 3
        text = G.join_lines(lines, np.random.default_rng(sep[0]))
        assert text.splitlines() == lines
        out.append(dict(mode="split", sep=sep[0], text=text, _name="table"))
        out.append(dict(mode="split", sep=sep[0], text=text.rstrip(b"\r\n"), _name="table_unterminated"))
    # more lines than one trip of a one-CU grid holds (16 workgroups x 256), the last wave partial
    lines = [b"k%d v%d" % (i, i) if i % 3 else b"junk%d" % i for i in range(4200)]
    out.append(dict(mode="split", sep=32, cus=1, text=b"\n".join(lines), _name="second_trip"))
    return out
