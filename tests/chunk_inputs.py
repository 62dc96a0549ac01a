"""One small batch that puts every seam of the chunk front end (k-mer-count_amd/csrc/kmc_chunks.hip.h) in front of every
kernel that uses it (tests/test_chunk_front_host.py checks the batch, tests/test_chunk_front_gpu.py runs it).  CPU only;
nothing here touches the library.

The kernels cut a batch into chunks of 1024 positions, 16 per lane; a wave holds 64 read starts at a time.  seam_batch(k)
is a little over five chunks:

  [0, 1024)       reads of 0 to 8 bases: hundreds of read starts in one chunk, a non-ACGT byte at 1023
  [1024, 1500)    a read that starts exactly at a chunk's first position, with a non-ACGT byte there
  1500            a run of 75 empty reads at one position
  [1500, 2064)    a read over the chunk edge at 2048 with a non-ACGT byte at 2051 - k: the first base of the window that
                  ends at 2050
  [2064, 3072)    a read that starts at a lane's first position (2048 + 16) and ends exactly at a chunk's end
  [3072, 5203)    one read of 2 * 1024 + 83 bases without a break, over the chunk edges at 4096 and 5120
  [5203, 5211)    a last read; 5211 is no multiple of 16

The text from 2606 on is a copy of the text from 0 on (made before the non-ACGT bytes go in, so the copy has none): the long
read repeats what the reads before it say, and counts above 1 occur."""
import numpy as np

CHUNK = 1024
LANE = 16
HELD = 64            # read starts a wave holds at a time
N_BASES = 5211
TINY_END = 1024      # the reads of 0 to 8 bases end here
EMPTY_AT = 1500
N_EMPTY = 75
LANE_START = 2 * CHUNK + LANE
LONG_BEGIN, LONG_END = 3 * CHUNK, 5203


def bad_positions(k):
    """where seam_batch(k) holds a non-ACGT byte"""
    return [CHUNK - 1, CHUNK, 2 * CHUNK + 3 - k]


def seam_batch(k, seed=0):
    """(bases u8[N_BASES], offsets u64[n_reads + 1]) for k in 5..63"""
    assert 5 <= k <= 63
    rng = np.random.default_rng(1000 * seed + k)
    half = N_BASES // 2 + 1
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, N_BASES)].copy()
    text[half:] = text[:N_BASES - half]
    for p, c in zip(bad_positions(k), b"NnR"):
        text[p] = c
    starts, p = [], 0
    while p < TINY_END:
        starts.append(p)
        p = min(p + int(rng.integers(0, 9)), TINY_END)
    starts += [TINY_END] + [EMPTY_AT] * (N_EMPTY + 1) + [LANE_START, LONG_BEGIN, LONG_END]
    return text, np.array(starts + [N_BASES], np.uint64)


def reads_of(bases, offs):
    """the batch as a list of strings (what the map model takes)"""
    raw = bytes(bases).decode()
    return [raw[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]
