#!/usr/bin/env python3
"""compare_csi.py OURS.csi THEIRS.csi -- a .csi `strling bamindex --csi` wrote against the one `samtools index -c` wrote for the
same BAM.  Equal: scheme, n_ref, per-reference pseudo-bin (file span, mapped / unmapped counts), n_no_coor, and the loffset of
every bin both files hold.  Chunks modulo htslib's compress_binning (which moves the chunks of small bins into their parents and
merges neighbours in one block): every chunk of ours must lie inside a chunk of theirs in the same bin or in one of its ancestors,
compared by compressed block offset.  Exit 0 when all of that holds; prints the first differences otherwise."""
import gzip
import struct
import sys


def parse(path):
    d = gzip.open(path, "rb").read()           # BGZF is a series of gzip members
    assert d[:4] == b"CSI\1", f"{path}: not a CSI index"
    m, depth, l_aux, = struct.unpack_from("<iii", d, 4)
    o = 16 + l_aux
    n_ref = struct.unpack_from("<i", d, o)[0]; o += 4
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", d, o)[0]; o += 4
        bins = {}
        for _ in range(n_bin):
            b, loff, nc = struct.unpack_from("<IQi", d, o); o += 16
            bins[b] = (loff, [struct.unpack_from("<QQ", d, o + 16 * k) for k in range(nc)]); o += 16 * nc
        refs.append(bins)
    no_coor = struct.unpack_from("<Q", d, o)[0] if o + 8 <= len(d) else None
    return (m, depth), refs, no_coor


def main(ours, theirs):
    (sa, ra, na), (sb, rb, nb) = parse(ours), parse(theirs)
    bad = []
    if sa != sb or len(ra) != len(rb) or na != nb:
        bad.append(f"scheme / n_ref / n_no_coor: {sa} {len(ra)} {na} against {sb} {len(rb)} {nb}")
    meta = ((1 << 3 * (sa[1] + 1)) - 1) // 7 + 1
    for t, (a, b) in enumerate(zip(ra, rb)):
        if a.get(meta) != b.get(meta):
            bad.append(f"reference {t}: pseudo-bin {a.get(meta)} against {b.get(meta)}")
        for k, (loff, chunks) in a.items():
            if k == meta:
                continue
            if k in b and b[k][0] != loff:
                bad.append(f"reference {t} bin {k}: loffset {loff} against {b[k][0]}")
            anc, x = [k], k
            while x:
                x = (x - 1) >> 3
                anc.append(x)
            for c0, c1 in chunks:
                if not any((p0 >> 16) <= (c0 >> 16) and (c1 >> 16) <= (p1 >> 16) + 1 for q in anc if q in b for p0, p1 in b[q][1]):
                    bad.append(f"reference {t} bin {k}: chunk ({c0}, {c1}) lies in no chunk of theirs in the bin or its ancestors")
    for line in bad[:20]:
        print(line)
    print("CSI: equal modulo compress_binning" if not bad else f"CSI: {len(bad)} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
