// The lane body of jpeg.hip's jpeg_ffcount_strips_kernel, included into it (and into tools/jpeg_ffcount_hostsim, where a
// host compiler reads the same text): the 0xff bytes of the scan's bit string that block `blk` OWNS, counted from the
// per-block strips without the packed string.  The includer provides
//     const uint32_t *strip            [word][nblk]: block b's word k at strip[k * nblk + b], MSB first, left-aligned
//     const uint32_t *nbits            [nblk] bits of every block's code (> 0)
//     const unsigned long long *pos    [nblk] exclusive prefix sum of nbits: the block's first bit in the string
//     int nblk, blk                    blk < nblk
//     uint32_t count                   += the owned bytes that equal 0xff
// Ownership: byte k of the string (bits 8k .. 8k + 7) belongs to the block that holds its FIRST bit, 8k in [p0, p1).  The
// blocks partition the string, so every byte has exactly one owner.  An owned byte's bits below p1 are the lane's own; the
// bits from p1 on are the top of the following blocks' word 0 (a block is 4 bits at the least -- chrominance DC category 0
// plus EOB --, so a byte can span three blocks), and behind the last block they are ones: writer.go's emit(0x7f, 7), whose
// padded byte can itself be 0xff.
{
    const unsigned long long p0 = pos[blk];
    const uint32_t nb = nbits[blk];
    const uint32_t skip = static_cast<uint32_t>((8u - static_cast<uint32_t>(p0 & 7u)) & 7u);   // own bits before the first owned byte
    if (nb > skip) {
        const int nw = static_cast<int>((nb + 31u) >> 5);
        unsigned long long acc = 0;          // MSB-first window: the low `have` bits are pending
        uint32_t have = 0;
        for (int k = 0; k < nw; k++) {
            const uint32_t w = strip[static_cast<size_t>(k) * static_cast<size_t>(nblk) + static_cast<size_t>(blk)];
            uint32_t valid = nb - 32u * static_cast<uint32_t>(k);
            if (valid > 32u) valid = 32u;
            acc = (acc << valid) | static_cast<unsigned long long>(w >> (32u - valid));
            have += valid;
            if (k == 0) have -= skip;        // the bits of the previous owner's byte drop off the window's top
            while (have >= 8u) {
                have -= 8u;
                count += ((acc >> have) & 0xffu) == 0xffu ? 1u : 0u;
            }
        }
        if (have > 0u) {
            // the byte that straddles p1: `have` own bits on top, the rest from the blocks behind -- which can only make
            // 0xff of it when the own bits are all ones
            uint32_t byte = static_cast<uint32_t>(acc) & ((1u << have) - 1u);
            if (byte == (1u << have) - 1u) {
                uint32_t need = 8u - have;
                for (int nx = blk + 1; need > 0u; nx++) {
                    if (nx >= nblk) {        // the padding
                        byte = (byte << need) | ((1u << need) - 1u);
                        break;
                    }
                    const uint32_t n2 = nbits[nx];
                    if (n2 == 0u) continue;
                    const uint32_t t = n2 < need ? n2 : need;
                    byte = (byte << t) | (strip[nx] >> (32u - t));
                    need -= t;
                }
                count += byte == 0xffu ? 1u : 0u;
            }
        }
    }
}
