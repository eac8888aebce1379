"""MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:329-403), restated sequentially from :365-397 for a list of
descriptors that the caller has gathered (the loop at :348-363 stays with the caller).  The statements follow the reference line for
line: the symmetric matrix with its zero diagonal, a sorted copy of every row, the element at int(0.5 * (N - 1)), the strict <."""
import numpy as np

INT_MAX = 2 ** 31 - 1
_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int32)


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:2256-2272): the number of differing bits of two 32-byte descriptors"""
    return int(_POPCOUNT[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum())


def distance_matrix(v):
    """Distances[N][N] of :371-381.  Short lists: the two loops as written; long ones: the same numbers from the popcount table"""
    N = len(v)
    if N <= 32:
        D = [[0] * N for _ in range(N)]
        for i in range(N):
            D[i][i] = 0                                        # :374
            for j in range(i + 1, N):                          # :375
                distij = descriptor_distance(v[i], v[j])       # :377
                D[i][j] = distij                               # :378
                D[j][i] = distij                               # :379
        return D
    v = np.asarray(v, np.uint8).reshape(N, 32)
    D = np.zeros((N, N), np.int32)
    for i in range(N):
        D[i] = _POPCOUNT[np.bitwise_xor(v[i][None, :], v)].sum(axis=1)
    return D.tolist()


def compute_distinctive_descriptor(v):
    """v: vDescriptors, [N, 32] uint8 -> (BestIdx, BestMedian); (-1, -1) for an empty list (the reference returns at :365)"""
    if len(v) == 0:                                            # :365
        return -1, -1
    N = len(v)                                                 # :369
    Distances = distance_matrix(v)
    BestMedian = INT_MAX                                       # :384
    BestIdx = 0                                                # :385
    for i in range(N):                                         # :386
        vDists = sorted(Distances[i][:N])                      # :388-389
        median = vDists[int(0.5 * (N - 1))]                    # :390
        if median < BestMedian:                                # :392
            BestMedian = median                                # :394
            BestIdx = i                                        # :395
    return BestIdx, BestMedian


def distinctive_descriptors(offsets, descriptors, out_descriptors=None):
    """The loop over the points of a call: -> (best_index [P], best_median [P], descriptors [P, 32]); the row of a point with an
    empty list stays what out_descriptors holds (zeros without one): mDescriptor is not touched"""
    offsets = np.asarray(offsets, np.int64)
    descriptors = np.asarray(descriptors, np.uint8).reshape(-1, 32)
    P = len(offsets) - 1
    idx, med = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    out = np.zeros((P, 32), np.uint8) if out_descriptors is None else np.array(out_descriptors, np.uint8).reshape(P, 32)
    for p in range(P):
        v = descriptors[offsets[p]:offsets[p + 1]]
        idx[p], med[p] = compute_distinctive_descriptor(v)
        if idx[p] >= 0:
            out[p] = v[idx[p]]                                 # :401
    return idx, med, out
