// rt_beam_lists.inl -- k_beam_lists_build: the beam lists of a still camera (rt_beam_lists.h: membership, dmin, the one arithmetic host and device share;
// rt_wide_format.h: the format), one wave per tile.  Included by rt_trace.hip behind rt_trace_packet.inl, whose front end scans the lists.
//
// A block is ONE wave and builds one tile: its pixel bounds from the tile's (up to) 64 entries of the slot -> pixel table -- no assumption of 8 x 8 alignment, of
// frame sizes that divide by 8 or of one shard -- then the walk of the 4-wide tree in rounds: up to RT_BEAM_ROUND pending nodes = 64 child records, one per lane;
// interior children whose stored box the tile's planes do not exclude go back on the pending stack (LDS), leaves whose EXACT box they do not exclude into the
// list (LDS), both in lane order; the list is ranked by (dmin, reference) and written out in that order.  Overflow of either gives the tile "no list".
// Cost: one launch of numTiles blocks per still camera; the break-even in passes stands next to the policy (rt_runtime_render.inl, beamListsFor).
#ifdef RT_DEVICE_KERNELS
__global__ void __launch_bounds__(64) k_beam_lists_build(const WideBvh bvh, const uint32_t* __restrict__ slotPixel, uint32_t numSlots, const BeamCamera cam, uint32_t capacity,
                                                         BeamEntry* __restrict__ entries, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t sStack[RT_BEAM_STACK];
    __shared__ BeamEntry sList[RT_BEAM_MAX_CAPACITY];
    __shared__ uint32_t sBounds[4];   // x0, x1, y0, y1
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    if (lane < 4u) sBounds[lane] = (lane & 1u) ? 0u : 0xFFFFu;
    if (lane == 0u) sStack[0] = 0u;   // node 0 holds the children of the binary tree's root
    __syncthreads();
    const uint32_t slot = tile * 64u + lane;
    if (slot < numSlots)
    {
        const uint32_t pix = slotPixel[slot], x = pix & 0xFFFFu, y = pix >> 16;
        atomicMin(&sBounds[0], x); atomicMax(&sBounds[1], x); atomicMin(&sBounds[2], y); atomicMax(&sBounds[3], y);
    }
    __syncthreads();
    const BeamPlanes planes = beamTilePlanes(cam, sBounds[0], sBounds[1], sBounds[2], sBounds[3]);
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t sp = 1u, count = 0u;   // block-uniform, as is `over`
    bool over = false;
    while (sp != 0u)
    {
        const uint32_t take = sp < RT_BEAM_ROUND ? sp : RT_BEAM_ROUND;
        sp -= take;
        BeamChild ch; ch.interior = false; ch.leaf = false; ch.ref = 0u; ch.dmin = 0.0f;
        if (lane < 4u * take) ch = beamClassify(bvh.nodes[4u * (size_t)sStack[sp + (lane >> 2)] + (lane & 3u)], bvh.gate, bvh.base, bvh.step, planes, cam);
        __syncthreads();   // the round's nodes are read: their places may be written
        const unsigned long long mI = __ballot(ch.interior), mL = __ballot(ch.leaf);
        const uint32_t numI = (uint32_t)__popcll(mI), numL = (uint32_t)__popcll(mL);
        if (sp + numI > RT_BEAM_STACK || count + numL > capacity) { over = true; break; }
        if (ch.interior) sStack[sp + (uint32_t)__popcll(mI & below)] = ch.ref;
        if (ch.leaf) sList[count + (uint32_t)__popcll(mL & below)] = BeamEntry{ ch.ref, __float_as_uint(ch.dmin) };
        sp += numI; count += numL;
        __syncthreads();
    }
    if (over) { if (lane == 0u) counts[tile] = RT_BEAM_NO_LIST; return; }
    if (lane < count)
    {
        const BeamEntry mine = sList[lane];
        uint32_t rank = 0u;
        for (uint32_t j = 0; j < count; ++j) if (beamEntryBefore(sList[j], mine)) rank++;
        entries[(size_t)tile * capacity + rank] = mine;   // (rank < count <= capacity: the order is total, two entries never share a leaf)
    }
    if (lane == 0u) counts[tile] = count;
}
#endif   // RT_DEVICE_KERNELS
