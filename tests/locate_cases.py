"""The cases of the locate, verify and MPHF lookup kernels (k_get_locate,
k_verify_*, k_lookup, k_sign, k_index_scatter and their device functions) run
on the host under ASan + UBSan (tests/test_locate_host_cpu.py) and, the valid
ones, on the GPU (tests/test_locate_cases_gpu.py); and the restatement both
compare with.  Not a test module: pure functions over numpy and the CPU oracle,
no device and no subprocess.  A case is a dict; the keys that start with "_"
are for the test's own reference and are not sent to the program.

Everything is restated here, the host program computes no truth:
  addresses   `decode` (get_plan.hpp::get_decode: compact -- partition = bits
              56..62, offset = low 56 bits, limit = the file's size; blocked
              (BlockedKVReader) -- block = bits 16..47 x 4096, bytes = bits
              48..55 x 4096, rec = low 16 bits, limit = the block's end, not the
              file's) and `record_rule` / `header_rule` (the 3-byte header and
              the whole record against that limit, then the key compare)
  the image   `layout` (get_plan.hpp::get_layout: 16-byte aligned bases, total
              = the last end rounded up to 16), filled from partition files that
              bsdb_amd.kvfiles wrote
  the MPHF    oracle.gov_build / oracle.lookup_batch; signatures from
              oracle.hash_var (the same hash for the three key readers)
  the rest    locate_expected, verify_expected, sign_expected, scatter_expected

What the host emulation proves: addressing, arithmetic, uniform control flow.
What it does not: the memory model, races between lanes, code generation,
speed -- the GPU suite stays the judge of the real kernels.

Key buffers (include/bsdb_mi355x.h): bsdb_dev_db_locate_* takes its keys "as for
bsdb_dev_verify_* (fixed-length keys at a 4-byte aligned address)", and those
"as in bsdb_dev_hash_*", where "d_blob may start at any address".  So `kmis` of
a fixed-length case is one of 0, 4, 8, 12, and a variable-length blob is tried
at every kmis of 0 .. 15.  Signatures of bsdb_dev_lookup / bsdb_dev_sign "must
be 16-byte aligned (a signature is read as one 16-byte pair)"."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle as O  # noqa: E402
from bsdb_amd import kvfiles  # noqa: E402

FOUND, REJECTED, KEY_MISMATCH, BAD_ADDR = 0, 1, 2, 3
PAGE = 4096
FILE_MASK = (1 << 56) - 1
U64 = (1 << 64) - 1
NS = (0, 1, 2, 63, 64, 65, 257, 3001)
NQS = (0, 1, 63, 64, 65, 255, 256, 257)
WIDTHS = (0, 1, 4, 7, 8, 13, 31, 32, 33, 63, 64)
FIXED_LENS = (1, 7, 8, 9, 16, 17, 32, 33, 255)
TAIL_LENS = (1, 7, 8, 9, 15, 16, 17)          # the key compare's last step: low_bytes_mask of 1 .. 8 bytes


# ---- the restatement: addresses ----------------------------------------------------------------------------------

def record_rule(f, limit, pos, key):
    """(status, position of the value, its length) of a record at `pos` of the partition file `f` whose container
    ends at `limit`, asked for `key`."""
    if pos + 3 > limit:
        return BAD_ADDR, 0, 0
    klen, vlen = int(f[pos]), int(f[pos + 1]) << 8 | int(f[pos + 2])
    if pos + 3 + klen + vlen > limit:
        return BAD_ADDR, 0, 0
    if bytes(f[pos + 3: pos + 3 + klen]) == bytes(key):
        return FOUND, pos + 3 + klen, vlen
    return KEY_MISMATCH, 0, 0


def header_rule(f, size, pos, key):
    """The status the header's rule gives a record at `pos` of a compact partition file `f` for `key`."""
    return record_rule(f, size, pos, key)[0]


def decode(word, fmt, sizes):
    """(partition, record position, container end), both offsets into the partition file; None: BAD_ADDR."""
    if word >> 63:
        return None
    part = word >> 56
    if part >= len(sizes):
        return None
    size = sizes[part]
    if fmt == 0:
        pos, limit = word & FILE_MASK, size
    else:
        block, nbytes, rec = ((word >> 16) & 0xFFFFFFFF) * PAGE, ((word >> 48) & 0xFF) * PAGE, word & 0xFFFF
        if nbytes == 0 or block + nbytes > size or rec + 3 > nbytes:
            return None
        pos, limit = block + rec, block + nbytes
    return (part, pos, limit) if pos + 3 <= limit else None


def layout(sizes):
    """(bases, total) of get_layout."""
    end, base = 0, []
    for s in sizes:
        base.append(end)
        end = (end + s + 15) // 16 * 16
    return base, end


class Image:
    """Partition files as the open lays them out in one allocation (pad bytes 0)."""

    def __init__(self, files, fmt=0, block=0):
        self.files, self.fmt, self.block = [bytes(f) for f in files], fmt, block
        self.sizes = [len(f) for f in self.files]
        self.base, self.total = layout(self.sizes)
        buf = bytearray(self.total)
        for b, f in zip(self.base, self.files):
            buf[b: b + len(f)] = f
        self.bytes = bytes(buf)

    def slot(self, word, key):
        """(status, src, vlen) of the index word (host order) for `key`: the rule over the partition's file alone."""
        d = decode(word, self.fmt, self.sizes)
        if d is None:
            return BAD_ADDR, 0, 0
        part, pos, limit = d
        st, vpos, vl = record_rule(self.files[part], limit, pos, key)
        return (st, self.base[part] + vpos, vl) if st == FOUND else (st, 0, 0)

    def container(self, word):
        """[lo, hi) of the image the record of this word may be read from; None when the decode refuses it."""
        d = decode(word, self.fmt, self.sizes)
        if d is None:
            return None
        part, pos, limit = d
        lo = 0 if self.fmt == 0 else limit - ((word >> 48) & 0xFF) * PAGE
        return self.base[part] + lo, self.base[part] + limit

    def outside_inverted(self, span):
        """The image with every byte outside `span` (None: every byte) inverted."""
        a = np.frombuffer(self.bytes, np.uint8).copy()
        inv = ~a
        if span is not None:
            inv[span[0]: span[1]] = a[span[0]: span[1]]
        return inv.tobytes()


def pack(items):
    off = np.zeros(len(items) + 1, np.uint64)
    if items:
        off[1:] = np.cumsum([len(k) for k in items])
    return np.frombuffer(b"".join(items), np.uint8) if items else np.zeros(0, np.uint8), off


def write_files(base, keys, vals, parts, fmt, block):
    kb, ko = pack(keys)
    vb, vo = pack(vals)
    if fmt == 0:
        return kvfiles.write_compact(base, parts, kb, ko, vb, vo)
    return kvfiles.write_blocked(base, parts, kb, ko, vb, vo, block)


def make_image(keys, vals, parts, fmt=0, block=PAGE):
    """(Image, every record's address) of these records; record i goes to partition i % parts."""
    with tempfile.TemporaryDirectory() as d:
        base = os.path.join(d, "kv.db")
        addr = write_files(base, keys, vals, parts, fmt, block)
        files = [open(f"{base}.{p}", "rb").read() for p in range(parts)]
    return Image(files, fmt, block if fmt else 0), [int(a) for a in addr]


def be(words):
    """Host-order words as the u64 whose bytes in memory are the big-endian address (an index.db slot)."""
    return [int(x) for x in np.array([int(w) for w in words], np.uint64).byteswap()]


# ---- the restatement: the MPHF ------------------------------------------------------------------------------------

def sigs_of(keys):
    return O.hash_var(*pack(keys)) if keys else np.zeros((0, 2), np.uint64)


def mph_of(sig, width):
    """The oracle's MPHF over these signatures, every array at exactly its documented length."""
    n = len(sig)
    if n == 0:
        E, values, sigbits = np.zeros(2, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    else:
        rc, E, values, sigbits = O.gov_build(sig, width)
        assert rc == 0
    assert E.size == O.num_buckets(n) + 1 and values.size == int(O.lib().bo_values_words(n))
    assert sigbits.size == (n * width + 63) // 64 + 1
    return dict(n=n, width=width, E=E, values=values, sigbits=sigbits)


def mph_args(mph):
    c = dict(n=mph["n"], width=mph["width"], E=mph["E"].tolist(), values=mph["values"].tolist())
    if mph["width"]:
        c["sigbits"] = mph["sigbits"].tolist()
    return c


def ranks(mph, sig, check=True):
    if len(sig) == 0:
        return np.zeros(0, np.int64)
    return O.lookup_batch(np.ascontiguousarray(sig, np.uint64), mph["n"], mph["E"], mph["values"], mph["width"],
                          mph["sigbits"], check)


def locate_grid(nq, cus):
    """get_locate_grid."""
    return max(1, min(-(-nq // 256), max(1, cus) * 16, 0xFFFFFFFF))


def grid_for(cus, n):
    """grid_for (gov_plan.hpp)."""
    return max(1, min((n + 255) // 256, cus * 16))


# ---- locate --------------------------------------------------------------------------------------------------------

def locate_case(name, mph, keys, kind, image=None, index=(), cus=2, kmis=0, mis=3, approx=False, image_bytes=None):
    """keys: the queries (bytes each); kind 0: 13-byte keys, 1: one length, 2: any lengths; index: host-order words."""
    blob, off = pack(keys)
    c = dict(mode="locate", **mph_args(mph), nq=len(keys), grid=locate_grid(len(keys), cus), kmis=kmis, mis=mis,
             keys=blob.tobytes(), index=be(index), approx=int(approx), _name=name, _mph=mph, _keys=list(keys),
             _index=[int(w) for w in index], _image=image, _kind=kind)
    if approx:
        c.update(image=b"", base=[], size=[], format=0)
    else:
        c.update(image=image.bytes if image_bytes is None else image_bytes, base=image.base, size=image.sizes, format=image.fmt)
        assert len(c["image"]) == image.total
    if kind == 2:
        c["off"] = off.tolist()
    else:
        lens = {len(k) for k in keys}
        assert kmis % 4 == 0 and len(lens) <= 1
        c["key_len"] = 13 if kind == 0 else (lens.pop() if lens else 8)
        assert (c["key_len"] == 13) == (kind == 0)
    return c


def locate_expected(c):
    """(status, src, vlen, the six report words) of a locate case."""
    r = ranks(c["_mph"], sigs_of(c["_keys"]))
    st, src, vl = [], [], []
    for key, rank in zip(c["_keys"], r):
        if rank < 0:
            s = (REJECTED, 0, 0)
        elif c["approx"]:
            s = (FOUND, int(rank), 8)
        else:
            s = c["_image"].slot(c["_index"][rank], key)
        st.append(s[0]), src.append(s[1]), vl.append(s[2])
    return st, src, vl, [len(st)] + [st.count(x) for x in range(4)] + [sum(vl)]


class Db:
    """A small database: keys, values, the oracle's MPHF over the keys, the image and a valid index."""

    def __init__(self, keys, vals, width, parts=1, fmt=0, block=PAGE, extra=()):
        """extra: (key, value) records written to the files after the others, of which the MPHF knows nothing."""
        self.keys, self.vals = list(keys), list(vals)
        self.parts, self.fmt, self.block = parts, fmt, block
        self.all_keys, self.all_vals = self.keys + [k for k, _ in extra], self.vals + [v for _, v in extra]
        self.mph = mph_of(sigs_of(self.keys), width)
        self.rank = ranks(self.mph, sigs_of(self.keys))
        n = len(self.keys)
        assert sorted(self.rank.tolist()) == list(range(n))
        if n:
            self.image, addr = make_image(self.all_keys, self.all_vals, parts, fmt, block)
        else:
            self.image, addr = Image([b""] * parts, fmt, block if fmt else 0), []
        self.addr = addr
        self.index = [0] * n
        for i in range(n):
            self.index[self.rank[i]] = addr[i]

    def index_a(self):
        """index_a.db's slots as u64 (W:140-142: the value's head, zero padded)."""
        out = [0] * len(self.keys)
        for i, v in enumerate(self.vals):
            out[self.rank[i]] = int.from_bytes(v[:8].ljust(8, b"\0"), "little")
        return out

    def write(self, d):
        """The kv files, index.db and index_a.db into directory d: (kv base, index path, index_a path)."""
        base = os.path.join(d, "kv.db")
        if self.keys:
            write_files(base, self.all_keys, self.all_vals, self.parts, self.fmt, self.block)
        else:
            for p in range(self.parts):
                open(f"{base}.{p}", "wb").close()
        np.array(self.index, ">u8").tofile(os.path.join(d, "index.db"))
        np.array(self.index_a(), "<u8").tofile(os.path.join(d, "index_a.db"))
        return base, os.path.join(d, "index.db"), os.path.join(d, "index_a.db")


def rand_bytes(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def distinct_keys(rng, n, lens):
    """n distinct keys whose lengths cycle through `lens` (each >= 1)."""
    out, seen, i = [], set(), 0
    while len(out) < n:
        k = rand_bytes(rng, lens[i % len(lens)])
        i += 1
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def twin(k):
    """The key that differs from k in its last byte only."""
    return k[:-1] + bytes([k[-1] ^ 0x80])


def absent(rng, present, count, lens):
    have, out = set(present), []
    while len(out) < count:
        k = rand_bytes(rng, lens[len(out) % len(lens)])
        if k not in have:
            out.append(k)
    return out


_memo = {}


def memo(f):
    def g(*a):
        if (f.__name__, a) not in _memo:
            _memo[(f.__name__, a)] = f(*a)
        return _memo[(f.__name__, a)]
    g.__name__ = f.__name__
    return g


LAYOUTS = (("compact3", 3, 0, PAGE), ("blocked4096", 2, 1, PAGE), ("compact1", 1, 0, PAGE), ("blocked8192", 2, 1, 2 * PAGE))


@memo
def db_by_n(n):
    """n variable-length keys (lengths 1 .. 40 mixed), values of 0 .. 20 bytes, the layouts in turn."""
    rng = np.random.default_rng(1000 + n)
    _, parts, fmt, block = LAYOUTS[NS.index(n) % 4]
    keys = distinct_keys(rng, n, list(range(2, 41)) + [1])
    vals = [rand_bytes(rng, l) for l in rng.integers(0, 21, n)]
    return Db(keys, vals, 13 if n == 3001 else 4, parts, fmt, block)


@memo
def db_by_width(width):
    """257 keys of 1 .. 17 bytes in three compact partitions whose sizes are no multiples of 16; the keys of TAIL_LENS
    bytes have a twin (the same bytes but the last) in the files that the MPHF does not know."""
    rng = np.random.default_rng(2000 + width)
    keys = distinct_keys(rng, 257, [3, 1, 7, 8, 9, 15, 16, 17, 5, 12])
    vals = [rand_bytes(rng, l) for l in rng.integers(0, 12, 257)]
    victims = [next(i for i, k in enumerate(keys) if len(k) == l and twin(k) not in keys) for l in TAIL_LENS]
    while True:
        db = Db(keys, vals, width, 3, 0, PAGE, extra=[(twin(keys[i]), b"tw") for i in victims])
        short = [p for p in (0, 1) if db.image.sizes[p] % 16 == 0]
        if not short:                         # pad bytes lie between the partitions
            break
        vals[short[0]] += b"x"
    for j, i in enumerate(victims):           # the victim's slot names its twin's record
        db.index[db.rank[i]] = db.addr[257 + j]
    db.victims = victims
    return db


@memo
def db_fixed(key_len):
    """Keys of one length behind a one-partition compact database; key_len 13 is kind 0."""
    rng = np.random.default_rng(3000 + key_len)
    n = 64 if key_len == 1 else 65
    keys = distinct_keys(rng, n, [key_len])
    return Db(keys, [rand_bytes(rng, l) for l in rng.integers(0, 9, n)], 7, 1, 0)


@memo
def db_values():
    """Value lengths 0, 1, 255, 256 and 65 535: (compact in three partitions, each ending with one of the long
    values; blocked 4096 with a block filled to its last byte and the longest value in a block of its own)."""
    rng = np.random.default_rng(4000)
    keys = [b"v%03d" % i for i in range(30)]
    lens = [0, 1, 255, 256] * 7 + [65535, 256]
    lens[27] = 255                            # records 27, 28, 29 end partitions 0, 1, 2
    vals = [rand_bytes(rng, l) for l in lens]
    compact = Db(keys, vals, 8, 3, 0)
    assert [s % 16 for s in compact.image.sizes] != [0, 0, 0]
    # blocked, one partition: records 0 .. 8 of 400 value bytes, record 9 fills block 0 to its last byte
    lens = [400] * 9 + [0] + [0, 1, 255, 256, 65535, 7]
    lens[9] = PAGE - sum(3 + 4 + 400 for _ in range(9)) - 3 - 4
    vals = [rand_bytes(rng, l) for l in lens]
    blocked = Db(keys[:16], vals, 8, 1, 1, PAGE)
    a = blocked.addr[9]
    assert (a & 0xFFFF) + 3 + 4 + lens[9] == PAGE == ((a >> 48) & 0xFF) * PAGE
    assert (blocked.addr[14] >> 48) & 0xFF == 17 and blocked.addr[14] & 0xFFFF == 0
    return compact, blocked


def queries_of(db, rng, n_absent, lens):
    """Every key of the database shuffled among absent ones (a zero-length key among them where lens has a 0)."""
    q = list(db.keys) + absent(rng, db.keys, n_absent, [l for l in lens if l] or [4]) + ([b""] if 0 in lens else [])
    return [q[i] for i in rng.permutation(len(q))]


@memo
def locate_valid():
    rng = np.random.default_rng(77)
    cases = []
    for n in NS:                              # the sizes of the MPHF, the layouts in turn, then approximate
        db = db_by_n(n)
        q = queries_of(db, rng, 40, list(range(0, 41)))[: 400 if n == 3001 else None]
        cases.append(locate_case(f"n{n}", db.mph, q, 2, db.image, db.index, cus=1))
        cases.append(locate_case(f"n{n}_approx", db.mph, q, 2, approx=True))
    for w in WIDTHS:                          # checksum widths; the twins (the compare's last step)
        db = db_by_width(w)
        q = queries_of(db, rng, 200, [1, 3, 7, 8, 9, 15, 16, 17])
        cases.append(locate_case(f"width{w}", db.mph, q, 2, db.image, db.index))
    empty = mph_of(np.zeros((0, 2), np.uint64), 0)       # n = 0 without checksum bits: every rank is n, none is a slot
    cases.append(locate_case("n0_width0", empty, q[:70], 2, db_by_n(0).image, []))
    db = db_fixed(8)                          # wave and workgroup edges; more queries than a grid of 16 has threads
    pool = db.keys + absent(rng, db.keys, 30, [8])
    for nq in NQS + (16 * 256 + 5,):
        q = [pool[i] for i in rng.integers(0, len(pool), nq)]
        cases.append(locate_case(f"nq{nq}", db.mph, q, 1, db.image, db.index, cus=1 if nq > 4096 else 2, kmis=4 * (nq % 4)))
    assert cases[-1]["grid"] * 256 < cases[-1]["nq"]
    db = db_fixed(13)                         # kind 0: nq = 4: the last key's window ends with the buffer; else it crosses
    pool = db.keys + absent(rng, db.keys, 10, [13])
    for nq in (1, 4, 5, 64, 65, 95):
        for kmis in (0, 4, 8, 12):
            q = [pool[i] for i in rng.permutation(len(pool))[:nq]]
            cases.append(locate_case(f"k13_nq{nq}_kmis{kmis}", db.mph, q, 0, db.image, db.index, kmis=kmis))
    for j, kl in enumerate(FIXED_LENS):       # kind 1
        db = db_fixed(kl)
        q = queries_of(db, rng, 20, [kl])
        cases.append(locate_case(f"fixed{kl}", db.mph, q, 1, db.image, db.index, kmis=4 * (j % 4)))
    db = db_by_n(65)                          # a variable-length blob at every address the header permits: any
    for kmis in range(1, 16):
        cases.append(locate_case(f"blob_kmis{kmis}", db.mph, queries_of(db, rng, 10, [0, 3, 9, 20]), 2, db.image, db.index, kmis=kmis))
    for db, name in zip(db_values(), ("values_compact", "values_blocked")):
        cases.append(locate_case(name, db.mph, queries_of(db, rng, 5, [4]), 2, db.image, db.index))
    return cases


# ---- lookup, sign, scatter, count ----------------------------------------------------------------------------------

def lookup_case(name, mph, sig, check, cus=2):
    sig = np.ascontiguousarray(sig, np.uint64).reshape(-1, 2)
    return dict(mode="lookup", **mph_args(mph), sig=sig.reshape(-1).tolist(), check=int(check), grid=grid_for(cus, len(sig)),
                _name=name, _mph=mph, _sig=sig)


def lookup_expected(c):
    return ranks(c["_mph"], c["_sig"], bool(c["check"])).tolist()


def sign_case(name, mph, sig, cus=2):
    sig = np.ascontiguousarray(sig, np.uint64).reshape(-1, 2)
    words = (len(sig) * mph["width"] + 63) // 64 + 1
    c = dict(mode="sign", **mph_args(mph), sig=sig.reshape(-1).tolist(), words=words, grid=grid_for(cus, len(sig)), _name=name,
             _mph=mph, _sig=sig)
    c.pop("sigbits", None)                    # the list is what k_sign makes
    return c


def sign_expected(c):
    """signatures[rank(sig)] = sig0 & mask as a packed width-bit list (GOV:492-508)."""
    w, words = c["width"], c["words"]
    bits = 0
    for (s0, _), r in zip(c["_sig"].tolist(), ranks(c["_mph"], c["_sig"], False).tolist()):
        bits |= (s0 & ((1 << w) - 1)) << (r * w)
    assert bits >> (64 * words) == 0
    return [(bits >> (64 * i)) & U64 for i in range(words)]


@memo
def mph_valid():
    """k_lookup (checked and not) and k_sign at every width and every n; the queries are the keys and absent ones."""
    rng = np.random.default_rng(5)
    cases = []
    for db in [db_by_width(w) for w in WIDTHS] + [db_by_n(n) for n in NS]:
        name = f"n{db.mph['n']}_w{db.mph['width']}"
        sig = sigs_of(db.keys + absent(rng, db.keys, 100, [5, 9]))
        for check in (1, 0):
            cases.append(lookup_case(f"lookup_{name}_{check}", db.mph, sig, check, cus=1))
        if db.mph["width"]:
            c = sign_case(f"sign_{name}", db.mph, sigs_of(db.keys))
            if db.keys:
                assert sign_expected(c) == db.mph["sigbits"].tolist()       # the oracle signed the same list
            cases.append(c)
    db = db_by_width(13)
    pool = sigs_of(db.keys + absent(rng, db.keys, 50, [6]))
    for nq in NQS + (16 * 256 + 5,):
        cases.append(lookup_case(f"lookup_nq{nq}", db.mph, pool[rng.integers(0, len(pool), nq)], 1, cus=1))
    return cases


def scatter_case(name, rank, addr, start, length, value8=None, value_len=None, cus=2, fill=0x11):
    c = dict(mode="scatter", rank=[int(r) for r in rank], addr=[int(a) for a in addr], start=start, len=length, fill=fill,
             grid=grid_for(cus, len(rank)), approx=int(value8 is not None), _name=name)
    if value8 is not None:
        c.update(value8=[int(v) for v in value8], value_len=[int(v) for v in value_len])
    return c


def scatter_expected(c):
    """(index words, index_a bytes): index[rank - start] = the byte-reversed address, and the first min(len, 8)
    value bytes (W:129-145); slots no rank names keep the fill."""
    fill = bytes([c["fill"]]) * 8
    index, index_a = [int.from_bytes(fill, "little")] * c["len"], bytearray(fill * c["len"]) if c["approx"] else bytearray()
    for i, r in enumerate(c["rank"]):
        if r < 0 or not c["start"] <= r < c["start"] + c["len"]:
            continue
        idx = r - c["start"]
        index[idx] = int.from_bytes(c["addr"][i].to_bytes(8, "little"), "big")
        if c["approx"]:
            l = min(c["value_len"][i], 8)
            index_a[8 * idx: 8 * idx + l] = c["value8"][i].to_bytes(8, "little")[:l]
    return index, bytes(index_a)


@memo
def scatter_valid():
    rng = np.random.default_rng(6)
    cases = []
    for start, length in ((0, 300), (100, 50), (5, 1), (7, 0)):
        inside = [start + j for j in range(length) if length < 6 or j not in (2, length // 2, length - 3)]   # distinct: one writer a slot
        rank = [-1, start - 1 if start else -1, start + length, start + length + 1, 1 << 40] + inside
        if length:
            assert start in rank and start + length - 1 in rank
        rank = [rank[i] for i in rng.permutation(len(rank))]
        addr = [int(x) for x in rng.integers(0, 1 << 63, len(rank), dtype=np.uint64)]
        v8 = [int(x) for x in rng.integers(0, 1 << 63, len(rank), dtype=np.uint64) * 2 + 1]
        vl = [(0, 7, 8, 9, 255)[i % 5] for i in range(len(rank))]
        cases.append(scatter_case(f"scatter_{start}_{length}", rank, addr, start, length))
        cases.append(scatter_case(f"scatter_a_{start}_{length}", rank, addr, start, length, v8, vl, cus=1))
    return cases


def count_case(name, values, spans, vmis=0):
    return dict(mode="count", values=[int(v) for v in values], span=[x for s in spans for x in s], vmis=vmis, _name=name,
                _spans=spans)


def count_expected(c):
    a = np.array(c["values"], np.uint64)
    return [O.count_nonzero_pairs(s, e, a) for s, e in c["_spans"]]


@memo
def count_valid():
    """Every start & 31 and end & 31 of 0, 1, 31, 0 .. 4 whole words between them, the first whole word at an even and
    at an odd word (the step up to a 16-byte boundary), the array at either 8-byte parity, `end` on and past the
    array's last pair (an exclusive end of 32 * words reads no word past the array)."""
    rng = np.random.default_rng(8)
    cases = []
    for words in (1, 2, 3, 8, 9):
        values = rng.integers(0, 1 << 63, words, dtype=np.uint64) * 2 + rng.integers(0, 2, words, dtype=np.uint64)
        values[rng.integers(0, words)] = 0
        spans = []
        for w0 in range(words):
            for so in (0, 1, 31):
                for whole in range(0, 5):
                    for eo in (0, 1, 31):
                        first_whole = w0 + (1 if so else 0)
                        s, e = 32 * w0 + so, 32 * (first_whole + whole) + eo
                        if s <= e and (e < 32 * words or (e == 32 * words and s < e)):
                            spans.append((s, e))
        spans += [(0, 32 * words - 1), (32 * words - 1, 32 * words - 1), (0, 32 * words)]
        for vmis in (0, 8):
            cases.append(count_case(f"count_{words}_{vmis}", values, spans, vmis))
    return cases


# ---- verify ----------------------------------------------------------------------------------------------------------

def verify_case(name, mph, keys, kind, index_full, start, length, addr=None, addr_base=0, addr_stride=0, first=0, value8=None,
                vlen=None, index_a_full=None, cus=2, kmis=0, no_values=False):
    """index_full / index_a_full: the n slots in host order (addresses) / as u64; the case carries the window's."""
    blob, off = pack(keys)
    c = dict(mode="verify", **mph_args(mph), count=len(keys), grid=grid_for(cus, len(keys)),
             sgrid=grid_for(cus, mph["E"].size), kmis=kmis, keys=blob.tobytes(), start=start, len=length,
             index=be(index_full[start: start + length]), addr_base=addr_base, addr_stride=addr_stride, first=first,
             _name=name, _mph=mph, _keys=list(keys), _index=[int(w) for w in index_full], _index_a=index_a_full)
    if no_values:
        c["no_values"] = 1
    if addr is not None:
        c["addr"] = [int(a) for a in addr]
    if index_a_full is not None:
        c.update(index_a=[int(w) for w in index_a_full[start: start + length]], value8=[int(v) for v in value8],
                 vlen=[int(v) for v in vlen])
    if kind == 2:
        c["off"] = off.tolist()
    else:
        c["key_len"] = len(keys[0]) if keys else 13 if kind == 0 else 8
        assert (c["key_len"] == 13) == (kind == 0) and kmis % 4 == 0
    return c


def structure_valid(E, n):
    """E[0]'s offset is 0, the offsets (low 56 bits) never decrease, E[m]'s is n."""
    off = [int(e) & FILE_MASK for e in E]
    return off[0] == 0 and off[-1] == n and all(a <= b for a, b in zip(off, off[1:]))


def verify_expected(c):
    """The eight report words: records, rejected, in_window, wrong_addr, wrong_value, min_bad, flags, windows."""
    mph = c["_mph"]
    if not structure_valid(mph["E"], mph["n"]):
        return [0, 0, 0, 0, 0, U64, 1, 0]
    r = ranks(mph, sigs_of(c["_keys"]))
    rej = inw = wa = wv = 0
    min_bad = U64
    for i, rank in enumerate(r.tolist()):
        ad = c["addr"][i] if "addr" in c else (c["addr_base"] + c["addr_stride"] * (c["first"] + i)) & U64
        bad = rank < 0
        rej += bad
        if rank >= 0 and c["start"] <= rank < c["start"] + c["len"]:
            inw += 1
            if c["_index"][rank] != ad:
                wa, bad = wa + 1, True
            if c["_index_a"] is not None:
                l = min(c["vlen"][i], 8)
                if (c["_index_a"][rank] ^ c["value8"][i]) & ((1 << (8 * l)) - 1):
                    wv, bad = wv + 1, True
        if bad:
            min_bad = min(min_bad, ad)
    return [len(c["_keys"]), rej, inw, wa, wv, min_bad, 0, 0]


@memo
def verify_valid():
    rng = np.random.default_rng(9)
    cases = []
    # the three kinds; addresses as an array and as base + stride * (first + i); the windows; a wrong address and a
    # wrong value each at the first record, the last record and a wave boundary
    for kind, db, kmis in ((2, db_by_width(13), 0), (1, db_fixed(9), 4), (0, db_fixed(13), 12), (2, db_by_n(3001), 0),
                           (2, db_by_n(0), 0), (2, db_by_n(1), 0)):
        n = len(db.keys)
        order = [int(i) for i in rng.permutation(n)]
        keys = [db.keys[i] for i in order]
        keys += absent(rng, db.keys, 3, [13 if kind == 0 else len(db.keys[0]) if kind == 1 else 6])
        # (absent: rejected, or accepted at another record's rank, which is a wrong address there)
        first, base, stride = 7, 1 << 40, 24
        addr = [base + stride * (first + i) for i in range(len(keys))]
        full = [0] * n
        for i, k in enumerate(order):
            full[db.rank[k]] = addr[i]
        v8 = [int(x) for x in rng.integers(0, 1 << 63, len(keys), dtype=np.uint64) * 2 + 1]
        vl = [(i + 3) % 10 for i in range(len(keys))]   # 0 .. 9; not 0 at the records made wrong below
        full_a = [0] * n
        for i, k in enumerate(order):          # the bytes past vlen in the slot differ from value8's
            l = min(vl[i], 8)
            full_a[db.rank[k]] = (v8[i] & ((1 << (8 * l)) - 1)) | ((~v8[i] & U64) >> (8 * l) << (8 * l) if l < 8 else 0)
        windows = [(0, n), (0, n // 2), (n // 2, n - n // 2), (n // 3, n // 3), (n, 0), (0, 0)] if n > 2 else [(0, n)]
        if n == 3001:                         # (several buckets: the whole window and one that cuts at both ends)
            windows = [(0, n), (n // 3, n // 3)]
        for start, length in windows:
            tag = f"verify_k{kind}_n{n}_{start}_{length}"
            cases.append(verify_case(tag, db.mph, keys, kind, full, start, length, addr=addr, kmis=kmis))
            cases.append(verify_case(tag + "_stride", db.mph, keys, kind, full, start, length, addr_base=base, addr_stride=stride,
                                     first=first, cus=1, kmis=kmis))
            cases.append(verify_case(tag + "_approx", db.mph, keys, kind, full, start, length, addr=addr, value8=v8, vlen=vl,
                                     index_a_full=full_a, kmis=kmis))
        if kind == 2 and n == 257:
            for k in range(1, 16):
                cases.append(verify_case(f"verify_blob_kmis{k}", db.mph, keys, 2, full, 0, n, addr=addr, kmis=k))
        if n > 64:
            for where in (0, 63, 64, n - 1):
                bad = list(full)
                bad[db.rank[order[where]]] ^= 1 << 17
                cases.append(verify_case(f"verify_k{kind}_n{n}_wrong_addr_{where}", db.mph, keys, kind, bad, 0, n, addr=addr, kmis=kmis))
                assert verify_expected(cases[-1])[3] == 1 and verify_expected(cases[-1])[5] == addr[where]
                bad_a = list(full_a)
                bad_a[db.rank[order[where]]] ^= 1 << (8 * (min(vl[where], 8) - 1))         # the last byte compared
                cases.append(verify_case(f"verify_k{kind}_n{n}_wrong_value_{where}", db.mph, keys, kind, full, 0, n, addr=addr,
                                         value8=v8, vlen=vl, index_a_full=bad_a, kmis=kmis))
                assert verify_expected(cases[-1])[4] == 1 and verify_expected(cases[-1])[5] == addr[where]
    return cases


def structure_case(name, E, n, cus=1):
    return dict(mode="structure", E=[int(e) for e in E], n=n, grid=grid_for(cus, len(E)), _name=name, _E=[int(e) for e in E])


# ---- hostile: index words against a fixed image ------------------------------------------------------------------

HOSTILE_LAYOUTS = (("compact", 3, 0, PAGE), ("blocked4096", 2, 1, PAGE), ("blocked8192", 2, 1, 2 * PAGE))
N_HOSTILE = 257


def planted(key, vb, body=b""):
    return bytes([len(key), vb >> 8, vb & 0xFF]) + key + body


@memo
def hostile_db(layout):
    """257 keys of 2 .. 12 bytes.  The values of records 30 .. 59 hold a whole record of their own key (a header
    planted in value bytes), those of records 60 .. 69 a record of their key's first bytes; the value of record 255 -- partition 0's last, and for the blocked layouts alone in its
    partition's last block -- holds three headers whose value lengths are set, once the files are written, so
    that the first (its own key) and the second (another key) end exactly with the container and the third one
    byte past it.  Compact: partitions 3 .. 6 are files of 0, 1, 2 and 3 bytes."""
    name, parts, fmt, block = next(l for l in HOSTILE_LAYOUTS if l[0] == layout)
    rng = np.random.default_rng({"compact": 11, "blocked4096": 12, "blocked8192": 13}[layout])
    keys = distinct_keys(rng, N_HOSTILE, list(range(2, 13)))
    vals = [rand_bytes(rng, l) for l in rng.integers(0, 40, N_HOSTILE)]
    for i in range(30, 60):
        vals[i] = planted(keys[i], 5, rand_bytes(rng, 5)) + rand_bytes(rng, 3)
    for i in range(60, 70):                   # ... and of their key without its last byte: the lengths differ
        vals[i] = planted(keys[i][:-1], 4, rand_bytes(rng, 4)) + keys[i][-1:]
    last = 255 if fmt == 0 else 256           # the last record of partition 0 (record i goes to partition i % parts)
    assert last % parts == 0 and last + parts >= N_HOSTILE
    k = keys[last]
    other = twin(k)
    tail = planted(k, 0) + planted(other, 0) + planted(k, 0) + rand_bytes(rng, 9)
    vals[last] = (rand_bytes(rng, block - 200) if fmt else b"") + tail      # blocked: too long for the block before it
    db = Db(keys, vals, 6, parts, fmt, block)
    f = bytearray(db.image.files[0])
    a = db.addr[last]
    pos = (a & FILE_MASK) if fmt == 0 else ((a >> 16) & 0xFFFFFFFF) * PAGE + (a & 0xFFFF)
    end = len(f) if fmt == 0 else ((a >> 16) & 0xFFFFFFFF) * PAGE + ((a >> 48) & 0xFF) * PAGE
    p = pos + 3 + len(k) + len(vals[last]) - len(tail)
    spots = []
    for j, over in enumerate((0, 0, 1)):
        vb = end - (p + 3 + len(k)) + over
        f[p + 1], f[p + 2] = vb >> 8, vb & 0xFF
        spots.append(p)
        p += 3 + len(k)
    files = [bytes(f)] + list(db.image.files[1:])
    if fmt == 0:
        files += [b"", b"\x01", b"\x00\x00", b"\x00\x00\x00"]
    db.image = Image(files, fmt, block if fmt else 0)
    db.last, db.spots = last, [s - pos for s in spots]        # the planted headers' distances from the record's start
    return db


def hostile_words(layout):
    """[(query record i, the word its slot holds, the class)] -- several words per class, any number per record."""
    db = hostile_db(layout)
    img, fmt = db.image, db.image.fmt
    rng = np.random.default_rng(len(layout))
    out = []
    some = [int(i) for i in rng.permutation(N_HOSTILE)]
    take = iter(some * 40)

    def add(cls, word, i=None):
        out.append((next(take) if i is None else i, word & U64, cls))

    for _ in range(40):
        add("random", int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2)))
    for i in some[:10]:
        add("sign_bit", db.addr[i] | 1 << 63, i)
    for i in some[10:20]:
        add("partition", (db.addr[i] & FILE_MASK) | len(img.sizes) << 56, i)
        add("partition", (db.addr[i] & FILE_MASK) | 127 << 56, i)
    for i in some[20:50]:                     # another record's valid address
        add("other_record", db.addr[(i + 3) % N_HOSTILE], i)
    for i in some[50:70]:
        for d in (1, 2, 3, 4, 8):
            add("near", db.addr[i] + d, i)
            add("near", db.addr[i] - d, i)
    for i in range(30, 60):                   # the record planted in the record's own value
        add("planted_record", db.addr[i] + 3 + len(db.keys[i]), i)
    for i in range(60, 70):
        add("planted_prefix", db.addr[i] + 3 + len(db.keys[i]), i)
    for spot in db.spots:                     # exactly at the container's end (own key, another key), one byte over
        add("planted_at_the_end", db.addr[db.last] + spot, db.last)
    if fmt == 0:
        for p, size in enumerate(img.sizes):
            for o in range(max(size - 4, 0), size + 2):
                add("compact_end", p << 56 | o)
        for p in (3, 4, 5, 6):
            for o in range(4):
                add("tiny_partition", p << 56 | o)
    else:
        pages = db.block // PAGE
        size_pages = [s // PAGE for s in img.sizes]
        for i in some[70:80]:
            add("bytes_0", db.addr[i] & ~(0xFF << 48), i)
        for p in range(2):
            for b in range(0, size_pages[p], pages):
                for rec in (db.block - 4, db.block - 3, db.block - 2, db.block - 1, db.block, 0xFFFF):
                    add("header_at_the_block_end", p << 56 | pages << 48 | b << 16 | rec)
            add("block_past_the_file", p << 56 | pages << 48 | (size_pages[p] + 1) << 16 | 10)
            add("block_past_the_file", p << 56 | pages << 48 | size_pages[p] << 16 | 10)
            add("block_past_the_file", p << 56 | (pages + 1) << 48 | (size_pages[p] - pages) << 16 | 10)
            add("block_past_the_file", p << 56 | 255 << 48 | 0xFFFFFFFF << 16 | 10)
        ended = 0
        for i in some:                        # a block whose end is exactly the file's size: the partition's last block
            a = db.addr[i]
            if ((a >> 16) & 0xFFFFFFFF) + ((a >> 48) & 0xFF) == size_pages[a >> 56] and ended < 6:
                add("block_ends_the_file", a, (i + 1) % N_HOSTILE)
                add("block_ends_the_file", a + 1, i)
                ended += 1
        assert ended
        for i in some[80:110]:                # the same record through a block of twice the pages that holds it
            a = db.addr[i]
            b, rec, p = (a >> 16) & 0xFFFFFFFF, a & 0xFFFF, a >> 56
            if b >= pages and rec + db.block <= 0xFFFF:
                add("wider_block", p << 56 | 2 * pages << 48 | (b - pages) << 16 | (rec + db.block), i)
            elif b + 2 * pages <= size_pages[p]:
                add("wider_block", p << 56 | 2 * pages << 48 | b << 16 | rec, i)
    return out


def hostile_rounds(layout):
    """The words dealt into rounds in which every record's slot holds at most one of them:
    [(the index of the round (host order), [(record, class)])]."""
    db = hostile_db(layout)
    rounds = []
    for i, word, cls in hostile_words(layout):
        r = next((r for r in rounds if i not in r[2]), None)
        if r is None:
            r = (list(db.index), [], set())
            rounds.append(r)
        r[0][db.rank[i]] = word
        r[1].append((i, cls))
        r[2].add(i)
    return [(idx, recs) for idx, recs, _ in rounds]


@memo
def hostile_index_cases(layout):
    """Per round: one case with every key as a query, then (containment) one case per container of the round's
    queries -- only the queries whose record the decode puts there, against an image in which every byte outside
    that container, the pad bytes included, is inverted.  _hostile: the queries whose slot holds a hostile word."""
    db = hostile_db(layout)
    cases = []
    for k, (idx, recs) in enumerate(hostile_rounds(layout)):
        c = locate_case(f"{layout}_round{k}", db.mph, db.keys, 2, db.image, idx)
        c["_hostile"] = [i for i, _ in recs]
        cases.append(c)
        groups = {}
        for i in range(N_HOSTILE):
            groups.setdefault(db.image.container(idx[db.rank[i]]), []).append(i)
        for span, members in sorted(groups.items(), key=lambda g: (g[0] is None, g[0])):
            c = locate_case(f"{layout}_round{k}_only_{span}", db.mph, [db.keys[i] for i in members], 2, db.image, idx,
                            image_bytes=db.image.outside_inverted(span))
            c["_hostile"] = [j for j, i in enumerate(members) if i in {r for r, _ in recs}]
            c["_span"] = span
            cases.append(c)
    return cases


# ---- hostile: offset arrays ------------------------------------------------------------------------------------------

def random_mph(rng, n, m, shape, width):
    """An offset array the structure check accepts over random values and checksum words, random seed bytes."""
    if shape == "one_bucket":
        off = [0] * (m // 2 + 1) + [n] * (m - m // 2)
    elif shape == "all_in_the_last":
        off = [0] * m + [n]
    elif shape == "empty_first_and_last":
        off = [0, 0] + sorted(int(x) for x in rng.integers(0, n + 1, m - 3)) + [n, n]
    else:
        off = [0] + sorted(int(x) for x in rng.integers(0, n + 1, m - 1)) + [n]
    E = np.array([o | int(s) << 56 for o, s in zip(off, rng.integers(0, 256, m + 1))], np.uint64)
    assert structure_valid(E, n)
    vw = int(O.lib().bo_values_words(n))
    return dict(n=n, width=width, E=E, values=rng.integers(0, 1 << 63, vw, dtype=np.uint64) * 2 + rng.integers(0, 2, vw, dtype=np.uint64),
                sigbits=rng.integers(0, 1 << 63, (n * width + 63) // 64 + 1, dtype=np.uint64) * 2)


@memo
def accepted_offset_cases():
    """k_lookup (checked and not), k_get_locate and k_verify_* over offset arrays that are valid but come from no
    build.  The oracle's C lookup takes every one of these shapes (it is run on them when the cases are made, here):
    none is left out of the comparison."""
    rng = np.random.default_rng(21)
    db = hostile_db("compact")
    keys = distinct_keys(rng, 300, [13])
    var_keys = distinct_keys(rng, 300, list(range(1, 30)))
    cases = []
    for shape in ("random", "one_bucket", "all_in_the_last", "empty_first_and_last"):
        for n, m, width in ((N_HOSTILE, 5, 0), (N_HOSTILE, 64, 5), (N_HOSTILE, 257, 64), (1, 4, 3)):
            mph = random_mph(rng, n, m, shape, width)
            tag = f"{shape}_n{n}_m{m}_w{width}"
            sig = rng.integers(0, 1 << 63, (300, 2), dtype=np.uint64) * 2 + 1
            for check in (1, 0):
                cases.append(lookup_case(f"lookup_{tag}_{check}", mph, sig, check))
            index = (db.index * 2)[:n]
            cases.append(locate_case(f"locate_{tag}", mph, var_keys, 2, db.image, index))
            cases.append(locate_case(f"locate13_{tag}", mph, keys, 0, db.image, index, kmis=4))
            addr = [int(x) for x in rng.integers(0, 1 << 62, 300)]
            cases.append(verify_case(f"verify_{tag}", mph, var_keys, 2, index, 0, n, addr=addr))
            cases.append(verify_case(f"verify13_{tag}", mph, keys, 0, index, n // 3, n - n // 3, addr_base=5, addr_stride=9, kmis=8,
                                     value8=addr, vlen=[i % 10 for i in range(300)], index_a_full=[int(x) for x in rng.integers(0, 1 << 62, n)]))
    return cases


@memo
def refused_offset_arrays():
    """[(name, E, n, whether the structure check must refuse it)]"""
    rng = np.random.default_rng(22)
    out = []
    for m in (1, 2, 64, 257):
        n = 40 * m
        good = [n * b // m for b in range(m + 1)]
        seeded = [o | int(s) << 56 for o, s in zip(good, rng.integers(1, 256, m + 1))]
        seeded[m - 1] |= 0xFF << 56
        for tag, base in (("", good), ("_seeded", seeded)):
            out.append((f"m{m}{tag}_valid", list(base), n, False))
            e = list(base)
            e[0] += 1
            out.append((f"m{m}{tag}_first_not_0", e, n, True))
            for b in sorted({0, 1, 63, 64, 255, 256, m - 1}):
                if b < m and (base[b + 1] & FILE_MASK) > 0:
                    e = list(base)
                    e[b] = (e[b] & ~FILE_MASK) | ((base[b + 1] & FILE_MASK) + 1)      # E[b] > E[b + 1]
                    out.append((f"m{m}{tag}_decrease_at_{b}", e, n, True))
            for d in (-1, 1):
                e = list(base)
                e[m] += d
                out.append((f"m{m}{tag}_last_is_n{d:+d}", e, n, True))
    return out


def decode_case(layout):
    """get_decode itself on every word of hostile_words and on every record's own address."""
    db = hostile_db(layout)
    words = [w for _, w, _ in hostile_words(layout)] + db.addr
    return dict(mode="decode", words=words, format=db.image.fmt, size=db.image.sizes, _name=f"decode_{layout}", _db=db)


def decode_expected(c):
    out = [decode(w, c["format"], c["size"]) for w in c["words"]]
    return [[int(d is not None) for d in out]] + [[d[j] if d else 0 for d in out] for j in range(3)]
