"""COCO's compressed counts string as pycocotools' rleToString and rleFrString read: the two plain loops, nothing else."""


def enc(counts) -> bytes:
    out = bytearray()
    for i, c in enumerate(counts):
        x = int(c) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            g = x & 31
            x >>= 5  # arithmetic
            more = x != -1 if g & 16 else x != 0
            out.append(g + (32 if more else 0) + 48)
    return bytes(out)


def dec(s) -> list:
    s = s.encode("ascii") if isinstance(s, str) else s
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            g = s[p] - 48
            x |= (g & 31) << (5 * k)
            more = bool(g & 32)
            p += 1
            k += 1
            if not more and g & 16:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts
