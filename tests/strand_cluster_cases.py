"""Numpy restatement of strand-blind clustering (include/meshclust_amd.h), shared
by test_cluster_strands_host.py and test_gpu_cluster_strands.py.  Nothing here calls the product.

  rc_perm(k)            rc(i) for every k-mer index (first base most significant, A 0 .. T 3)
  canon_rows(h, k)      canon[i] = row[i] + row[rc(i)] - 1
  orient(ha, hb, k)     (strand, sad_plus, sad_minus): minus iff sad_minus < sad_plus, a tie is plus
  revcomp / doubled     the reverse-complemented record, and r || N x 30 || rc(r), with segments
  flipped(i, T)         the flip rule of the planted fixtures: read i is reverse-complemented iff
                        (i // T) % 2 == 1 (every second read of each template)
"""
import numpy as np

N = ord("N")
GAP = 30


def rc_perm(k):
    i = np.arange(4 ** k, dtype=np.int64)
    r = np.zeros_like(i)
    x = i.copy()
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def canon_rows(h, k):
    h = np.asarray(h).astype(np.int64)
    return h + h[..., rc_perm(k)] - 1


def orient(ha, hb, k):
    """Rows of pairs (same shape) -> (strand uint8, sad_plus, sad_minus)."""
    ha = np.asarray(ha).astype(np.int64)
    hb = np.asarray(hb).astype(np.int64)
    plus = np.abs(ha - hb).sum(axis=-1)
    minus = np.abs(ha - hb[..., rc_perm(k)]).sum(axis=-1)
    return (minus < plus).astype(np.uint8), plus.astype(np.uint64), minus.astype(np.uint64)


def revcomp(codes, segs):
    """The reverse-complemented record with its segments mirrored (bytes outside 0..3 stay)."""
    codes = np.asarray(codes, np.uint8)
    L = len(codes)
    rev = codes[::-1]
    out = np.where(rev <= 3, 3 - rev, rev).astype(np.uint8)
    return out, sorted([L - 1 - e, L - 1 - s] for s, e in segs)


def doubled(codes, segs):
    """r || N x 30 || rc(r): its forward histogram is the canonical row of r."""
    codes = np.asarray(codes, np.uint8)
    L = len(codes)
    rc, rsegs = revcomp(codes, segs)
    out = np.concatenate([codes, np.full(GAP, N, np.uint8), rc])
    return out, [list(s) for s in segs] + [[L + GAP + s, L + GAP + e] for s, e in rsegs]


def flipped(i, T):
    return (i // T) % 2 == 1


def flip_fasta(src, dst, T):
    """Copy a FASTA (one header line and sequence lines per record) with read i reverse-
    complemented iff flipped(i, T); headers stay.  Returns the headers' first words."""
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    names, recs = [], []
    with open(src, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                names.append(line[1:].split()[0].decode())
                recs.append([line, []])
            elif line:
                recs[-1][1].append(line)
    with open(dst, "wb") as f:
        for i, (hdr, lines) in enumerate(recs):
            seq = b"".join(lines)
            if flipped(i, T):
                seq = seq.translate(comp)[::-1]
            f.write(hdr + b"\n")
            for j in range(0, len(seq), 60):
                f.write(seq[j:j + 60] + b"\n")
    return names
