"""The frame store as a host model (helper of test_frame_store_model_cpu.py and
test_frame_store_edges_gpu.py; plain numpy, no import of the library).

It restates the comment above k_frames_push (reth_amd/csrc/replay.hip), one statement per
sentence of it.  The state is what the device keeps:

    head    frames pushed so far, the next frame id (a Python int: ids pass 2^31 and 2^33)
    store   uint8 [F, frame_bytes], frame id f lives in row f % F
    sid     int32 [n * ring_slots, K], a frame-ring stack's K frame ids, each already mod F

Every write goes to id % F, so the model overwrites old frames exactly as the device does and a
comparison with the device is exact equality at any F -- also after the ring has wrapped over
frames that rows still point at.  One limit is the device's own: the frames of ONE push are
written by concurrent workgroups, so their order is only defined while they land in different
rows, i.e. while F is at least the frames of that push (n + dones, or K n at init); the model
refuses a push beyond that instead of picking an order.

The ring is the actors' frame ring, uint8 [n * ring_slots, K, ...]; stack handles (s0_h, s1_h)
index its first axis, actor i's slot c is stack i * ring_slots + c.
"""
import numpy as np


class FrameStoreModel:
    def __init__(self, n_frames, stack, frame_bytes, n_actors, ring_slots, head=0):
        self.F, self.K, self.fb = int(n_frames), int(stack), int(frame_bytes)
        self.n, self.slots = int(n_actors), int(ring_slots)
        self.head = int(head)
        self.store = np.zeros((self.F, self.fb), np.uint8)
        self.sid = np.zeros((self.n * self.slots, self.K), np.int32)

    def _ring(self, ring):
        ring = np.asarray(ring)
        assert ring.dtype == np.uint8 and ring.shape[:2] == (self.n * self.slots, self.K), (ring.dtype, ring.shape)
        return ring.reshape(self.n * self.slots, self.K, self.fb)

    def _fits(self, frames):
        if frames > self.F:
            raise ValueError(f"{frames} frames in one push into a store of {self.F}: their write order is undefined")

    def push_init(self, ring, cur_slot):
        """mode 1: actor i's current stack (slot cur_slot[i]) enters as the K new frames
        head + K i + k; sid of that stack is those ids mod F; head += K n"""
        ring = self._ring(ring)
        self._fits(self.K * self.n)
        for i in range(self.n):
            st = i * self.slots + int(cur_slot[i])
            for k in range(self.K):
                fid = self.head + self.K * i + k
                self.store[fid % self.F] = ring[st, k]
                self.sid[st, k] = fid % self.F
        self.head += self.K * self.n

    def push_step(self, ring, s0_h, s1_h, done, cur_slot):
        """mode 0: frame K-1 of stack s1_h[i] gets id head + i and
        sid[s1] = sid[s0][1:] ++ [(head + i) % F]; for a done actor, frame 0 of its reset stack
        i * ring_slots + cur_slot[i] gets id head + n + (done actors before i) and that stack's
        sid is the id K times; head += n + dones"""
        ring = self._ring(ring)
        done = np.asarray(done) != 0
        self._fits(self.n + int(done.sum()))
        rank = 0
        for i in range(self.n):
            h0, h1 = int(s0_h[i]), int(s1_h[i])
            fid = self.head + i
            self.store[fid % self.F] = ring[h1, self.K - 1]
            shifted = list(self.sid[h0, 1:]) + [fid % self.F]  # sid[s0] read before sid[s1] is written
            self.sid[h1] = shifted
            if done[i]:
                rs = i * self.slots + int(cur_slot[i])
                rid = self.head + self.n + rank
                self.store[rid % self.F] = ring[rs, 0]
                self.sid[rs] = rid % self.F
                rank += 1
        self.head += self.n + rank

    def gather(self, id_rows):
        """the stacks of id tuples [..., K] -> uint8 [..., K, frame_bytes]"""
        return self.store[np.asarray(id_rows, dtype=np.int64)]
