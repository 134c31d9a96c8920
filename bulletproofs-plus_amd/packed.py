"""Array forms of the batch entry points for large inputs (tens of thousands of proofs per call).

api.py mirrors the reference's object interface (one RangeStatement / RangeProof / RangeWitness object per proof) and
marshals item by item with ctypes, ~20 us per proof; a caller that already holds its proofs, commitments and openings
as contiguous arrays uses these instead: the bpp_verify_item / bpp_prove_item arrays of include/bpp.h are built with
numpy pointer arithmetic (no per-item Python), the calls are the same C ABI calls.

Shapes (n items, aggregation m, extension degree t, rounds = log2(m * bit_length)):
    proofs        uint8 [n, 1 + 32 (t + 5 + 2 rounds)]     RangeProof::to_bytes()          (src/range_proof.rs:1120-1150)
    commitments   uint8 [n, m, 32]                         statement.commitments_compressed (src/range_statement.rs:27)
    min_values    uint64 [n, m], min_present uint8 [n, m]  Option<u64> promises             (src/range_statement.rs:29)
    seed_nonces   uint8 [n, 32] or None                                                      (src/range_statement.rs:31)
    values        uint64 [n, m], blindings uint8 [n, m, t, 32]   RangeWitness openings      (src/commitment_opening.rs:14-37)
    rng_bytes     uint8 [n, 32 (rounds + 3)]               what the external RNG hands out  (src/range_proof.rs:232-608)
"""
import ctypes
import time
from ctypes import POINTER, byref, c_size_t, c_uint64

import numpy as np

from . import _lib, api

_VERIFY_ITEM = np.dtype([("proof", "<u8"), ("proof_len", "<u8"), ("commitments32", "<u8"), ("m", "<u4"), ("_pad", "<u4"),
                         ("min_values", "<u8"), ("min_present", "<u8"), ("seed_nonce32", "<u8"), ("transcript_state", "<u8"),
                         ("transcript_label", "<u8"), ("label_len", "<u8")])
_PROVE_ITEM = np.dtype([("values", "<u8"), ("blindings32", "<u8"), ("commitments32", "<u8"), ("m", "<u4"), ("_pad", "<u4"),
                        ("min_values", "<u8"), ("min_present", "<u8"), ("seed_nonce32", "<u8"), ("transcript_state", "<u8"),
                        ("transcript_label", "<u8"), ("label_len", "<u8"), ("rng_bytes", "<u8"), ("rng_len", "<u8")])
assert _VERIFY_ITEM.itemsize == ctypes.sizeof(_lib.VerifyItem) and _PROVE_ITEM.itemsize == ctypes.sizeof(_lib.ProveItem)


def _c(a, dtype, shape):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.shape != tuple(shape):
        raise api.ProofError(api.ProofErrorKind.InvalidLength, "array of shape %s expected, got %s" % (tuple(shape), a.shape))
    return a


def _rows(a):
    """addresses of the rows of a C-contiguous array"""
    return a.ctypes.data + np.arange(a.shape[0], dtype=np.uint64) * np.uint64(a.strides[0])


def commit(params, values, blindings):
    """PedersenGens::commit for k openings (src/generators/pedersen_gens.rs:112-122): uint64 [k], uint8 [k, nb, 32] -> [k, 32]"""
    values = np.ascontiguousarray(values, dtype=np.uint64)
    k = values.shape[0]
    blindings = np.ascontiguousarray(blindings, dtype=np.uint8)
    nb = blindings.shape[1]
    blindings = _c(blindings, np.uint8, (k, nb, 32))
    out = np.zeros((k, 32), dtype=np.uint8)
    eng = params.engine
    rc = eng.lib.bpp_pedersen_commit(eng.ctx, params.handle, values.ctypes.data, blindings.ctypes.data, nb, k, out.ctypes.data)
    api._check(rc, eng.ctx)
    return out


def prove(params, values, blindings, commitments, min_values, min_present, seed_nonces, label, rng_bytes):
    """n x RangeProof::prove_with_rng in one bpp_prove_batch call -> uint8 [n, proof_len]

    commitments=None: prove from the openings alone (bpp_prove_openings: the engine makes commit(v, r) for every opening and uses
    them as the statements' commitments) -> (commitments uint8 [n, m, 32], proofs uint8 [n, proof_len])"""
    n_bits, t = params.bit_length(), int(params.extension_degree())
    values = np.ascontiguousarray(values, dtype=np.uint64)
    n, m = values.shape
    rounds = max((n_bits * m).bit_length() - 1, 0)
    blindings = _c(blindings, np.uint8, (n, m, t, 32))
    if commitments is not None:
        commitments = _c(commitments, np.uint8, (n, m, 32))
    min_values = _c(min_values, np.uint64, (n, m))
    min_present = _c(min_present, np.uint8, (n, m))
    rng_bytes = _c(rng_bytes, np.uint8, (n, 32 * (rounds + 3)))
    lbl = np.frombuffer(bytes(label), dtype=np.uint8).copy() if len(label) else np.zeros(1, dtype=np.uint8)
    items = np.zeros(n, dtype=_PROVE_ITEM)
    items["values"] = _rows(values)
    items["blindings32"] = _rows(blindings)
    if commitments is not None:
        items["commitments32"] = _rows(commitments)
    items["m"] = m
    items["min_values"] = _rows(min_values)
    items["min_present"] = _rows(min_present)
    if seed_nonces is not None:
        seed_nonces = _c(seed_nonces, np.uint8, (n, 32))
        items["seed_nonce32"] = _rows(seed_nonces)
    items["transcript_label"] = lbl.ctypes.data
    items["label_len"] = len(label)
    items["rng_bytes"] = _rows(rng_bytes)
    items["rng_len"] = rng_bytes.shape[1]
    plen = 1 + 32 * (t + 5 + 2 * rounds)
    out = np.empty((n, plen), dtype=np.uint8)  # (every byte is written by the call, or the call raises)
    got = c_size_t()
    err = ctypes.create_string_buffer(256)
    eng = params.engine
    if commitments is None:
        made = np.empty((n, m, 32), dtype=np.uint8)
        lens = (c_size_t * n)()
        rc = eng.lib.bpp_prove_openings(eng.ctx, params.handle, items.ctypes.data_as(POINTER(_lib.ProveItem)), n, made.ctypes.data, 32 * m,
                                        out.ctypes.data, plen, lens, None, err, 256)
        api._check(rc, eng.ctx, err)
        return made, out
    rc = eng.lib.bpp_prove_batch(eng.ctx, params.handle, items.ctypes.data_as(POINTER(_lib.ProveItem)), n, out.ctypes.data, plen,
                                 byref(got), err, 256)
    api._check(rc, eng.ctx, err)
    assert got.value == plen
    return out


class PackedInput:
    """A homogeneous batch as contiguous arrays + the bpp_packed_batch that describes it (include/bpp.h).  Holds the
    arrays alive; `.struct` can be passed to any *_packed entry point any number of times."""

    def __init__(self, proofs, commitments, min_values, min_present, seed_nonces, label, seed_present=None, state=None):
        self.proofs = np.ascontiguousarray(proofs, dtype=np.uint8)
        n, plen = self.proofs.shape
        commitments = np.ascontiguousarray(commitments, dtype=np.uint8)
        m = commitments.shape[1]
        self.commitments = _c(commitments, np.uint8, (n, m, 32))
        self.min_values = None if min_values is None else _c(min_values, np.uint64, (n, m))
        self.min_present = None if min_present is None else _c(min_present, np.uint8, (n, m))
        self.seed_nonces = None if seed_nonces is None else _c(seed_nonces, np.uint8, (n, 32))
        self.seed_present = None if seed_present is None else _c(seed_present, np.uint8, (n,))
        self.label = np.frombuffer(bytes(label), dtype=np.uint8).copy() if len(label) else np.zeros(1, dtype=np.uint8)
        self.state = None if state is None else np.frombuffer(bytes(state), dtype=np.uint8).copy()
        self.n, self.m = n, m
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        self.struct = _lib.PackedBatch(n, ptr(self.proofs), plen, self.proofs.strides[0], ptr(self.commitments), m,
                                       ptr(self.min_values), ptr(self.min_present), ptr(self.seed_nonces),
                                       ptr(self.seed_present), ptr(self.state), ptr(self.label), len(label))


def verify_batch(params, inp, action=api.VerifyAction.VerifyOnly, chunk=api.MAX_RANGE_PROOF_BATCH_SIZE, states=False):
    """RangeProof::verify_batch over a PackedInput in ONE C call (bpp_verify_batch_packed: upload, verify, release).
    Returns (masks uint8 [n, t, 32], present uint8 [n]); with states=True (bpp_verify_batch_packed_states) a third array,
    uint8 [n, 203]: every proof's transcript as the verifier left it."""
    eng, t = params.engine, int(params.extension_degree())
    masks = np.zeros((inp.n, t, 32), dtype=np.uint8)
    present = np.zeros(inp.n, dtype=np.uint8)
    err = ctypes.create_string_buffer(256)
    if states:
        st = np.zeros((inp.n, 203), dtype=np.uint8)
        rc = eng.lib.bpp_verify_batch_packed_states(eng.ctx, params.handle, byref(inp.struct), int(action), chunk, masks.ctypes.data,
                                                    present.ctypes.data, st.ctypes.data, err, 256)
        api._check(rc, eng.ctx, err)
        return masks, present, st
    rc = eng.lib.bpp_verify_batch_packed(eng.ctx, params.handle, byref(inp.struct), int(action), chunk, masks.ctypes.data,
                                         present.ctypes.data, err, 256)
    api._check(rc, eng.ctx, err)
    return masks, present


class DevicePackedInput:
    """A homogeneous batch whose arrays already lie in DEVICE memory + the bpp_packed_batch that describes it, for the *_packed_device
    entry points (include/bpp.h): nothing is copied to the host, one kernel checks and packs the batch where it lies.

    Every array is a torch device tensor or an (address, shape) pair: uint8 tensors for bytes, any 8-byte dtype for min_values (torch's
    uint64 is thin: int64 bit patterns are what is expected).  proofs may be a view whose rows are further apart than their length
    (stride(0) >= proof length, or proof_stride= with an address).  Shapes, contiguity and the device index are checked here; the kind
    of memory behind the addresses is checked by the engine (bpp_device_pointer_check) before it launches anything.

    Ordering: what wrote the arrays must be ordered before the engine's stream.  order_before(engine) -- called by verify_batch_device and
    ResidentBatch(form="device") -- synchronises torch's current stream unless the engine was created on that very stream
    (Engine(stream=torch.cuda.current_stream().cuda_stream)); `.synchronised` says which it was.  With raw addresses the caller orders."""

    def __init__(self, proofs, commitments, min_values=None, min_present=None, seed_nonces=None, label=b"", seed_present=None, state=None,
                 proof_stride=None, item_states=None):
        self._keep, self.device_index, self._torch, self.synchronised = [], None, False, False
        addr_p, shape, stride = self._array(proofs, "proofs", 1, rows=True)
        if len(shape) != 2:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "proofs: an array of shape (n, proof_len) expected, got %s" % (shape,))
        n, plen = shape
        stride = int(proof_stride) if proof_stride is not None else (stride if stride is not None else plen)
        addr_c, cshape, _ = self._array(commitments, "commitments", 1)
        if len(cshape) != 3 or cshape[0] != n or cshape[2] != 32:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "commitments: an array of shape (%d, m, 32) expected, got %s" % (n, cshape))
        m = cshape[1]

        def opt(a, name, itemsize, want):
            if a is None:
                return None
            addr, got, _ = self._array(a, name, itemsize)
            if got != want:
                raise api.ProofError(api.ProofErrorKind.InvalidLength, "%s: array of shape %s expected, got %s" % (name, want, got))
            return addr

        self.label = np.frombuffer(bytes(label), dtype=np.uint8).copy() if len(label) else np.zeros(1, dtype=np.uint8)
        self.state = None if state is None else np.frombuffer(bytes(state), dtype=np.uint8).copy()
        self.n, self.m, self.proof_len = n, m, plen
        self.struct = _lib.PackedBatch(n, addr_p, plen, stride, addr_c, m, opt(min_values, "min_values", 8, (n, m)),
                                       opt(min_present, "min_present", 1, (n, m)), opt(seed_nonces, "seed_nonces", 1, (n, 32)),
                                       opt(seed_present, "seed_present", 1, (n,)), None if self.state is None else self.state.ctypes.data,
                                       self.label.ctypes.data, len(label))
        self._item_states(item_states, n, opt)

    def _item_states(self, item_states, n, opt):
        """item_states= (per-item transcripts, the *_transcripts calls of include/bpp.h): a uint8 [n, 203] device tensor (any byte
        address: a slice of a larger tensor will do) or an (address, (n, 203)) pair; row i is the STROBE state item i is verified under.
        Such an input goes through bpp_batch_upload_*_device_transcripts / bpp_batch_refill_enqueue*_transcripts: label and state
        are not passed on."""
        self.item_states = None if item_states is None else ctypes.c_void_p(opt(item_states, "item_states", 1, (n, 203)))

    def struct_without_transcript(self):
        """a copy of .struct with the transcript fields null, as the refills and the *_transcripts uploads want it"""
        st = type(self.struct).from_buffer_copy(self.struct)
        st.transcript_state, st.transcript_label, st.label_len = None, None, 0
        return st

    def _array(self, a, name, itemsize, rows=False):
        """-> (address, shape, row stride in bytes or None)"""
        if isinstance(a, tuple) and len(a) == 2 and not hasattr(a[0], "data_ptr"):
            return int(a[0]), tuple(int(d) for d in a[1]), None
        if not hasattr(a, "data_ptr") or not getattr(a, "is_cuda", False):
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "%s: a torch device tensor or an (address, shape) pair expected" % name)
        import torch
        if (itemsize == 1 and a.dtype != torch.uint8) or a.element_size() != itemsize:
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "%s: %s expected, got %s" % (name, "uint8" if itemsize == 1 else "an 8-byte dtype", a.dtype))
        if rows and a.dim() == 2:
            ok = a.shape[0] <= 1 or (a.stride(1) == 1 and a.stride(0) >= a.shape[1])
        else:
            ok = a.is_contiguous()
        if not ok:
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "%s: not contiguous" % name)
        index = a.device.index if a.device.index is not None else torch.cuda.current_device()
        if self.device_index is None:
            self.device_index = index
        elif self.device_index != index:
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "%s: on device %d, other arrays on device %d" % (name, index, self.device_index))
        self._keep.append(a)
        self._torch = True
        return a.data_ptr(), tuple(a.shape), (a.stride(0) if rows and a.dim() == 2 and a.shape[0] > 1 else None)

    def order_before(self, engine):
        """make what wrote the tensors ordered before `engine`'s stream; True when that took a synchronisation"""
        self.synchronised = False
        if self.device_index is not None and self.device_index != int(engine.device):
            raise api.ProofError(api.ProofErrorKind.InvalidArgument,
                                 "arrays on device %d, engine on device %d" % (self.device_index, int(engine.device)))
        if not self._torch:
            return False
        import torch
        cur = torch.cuda.current_stream(self.device_index)
        if engine.stream and int(cur.cuda_stream) == engine.stream:
            return False
        cur.synchronize()
        self.synchronised = True
        return True


def verify_batch_device(params, inp, action=api.VerifyAction.VerifyOnly, chunk=api.MAX_RANGE_PROOF_BATCH_SIZE):
    """verify_batch over a DevicePackedInput in ONE C call (bpp_verify_batch_packed_device): the results of verify_batch on the same
    bytes in host memory.  Returns (masks uint8 [n, t, 32], present uint8 [n]) (host arrays)."""
    eng, t = params.engine, int(params.extension_degree())
    masks = np.zeros((inp.n, t, 32), dtype=np.uint8)
    present = np.zeros(inp.n, dtype=np.uint8)
    err = ctypes.create_string_buffer(256)
    inp.order_before(eng)
    rc = eng.lib.bpp_verify_batch_packed_device(eng.ctx, params.handle, byref(inp.struct), int(action), chunk, masks.ctypes.data,
                                                present.ctypes.data, err, 256)
    api._check(rc, eng.ctx, err)
    return masks, present


def _host_array(a):
    """a numpy array of a numpy array or a host torch tensor"""
    if hasattr(a, "data_ptr"):
        if getattr(a, "is_cuda", False):
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "a host array expected, got a device tensor")
        a = a.numpy()
    return np.asarray(a)


def _mixed_meta(proof_lens, m):
    """proof_lens as size_t [n] and m as uint32 [n], host arrays in every form; -> (lens, m, n)"""
    lens = np.ascontiguousarray(_host_array(proof_lens), dtype=np.uintp)
    m = np.ascontiguousarray(_host_array(m), dtype=np.uint32)
    if lens.ndim != 1 or m.shape != lens.shape:
        raise api.ProofError(api.ProofErrorKind.InvalidLength, "proof_lens and m: two arrays of shape (n,) expected")
    return lens, m, lens.shape[0]


class MixedInput:
    """A batch of MIXED aggregation factors as arrays of rows + the bpp_mixed_batch that describes it (include/bpp.h): the geometry
    of what bpp_prove_batch_mixed / bpp_prove_openings write.  Rows are numpy arrays or host torch tensors:
        proofs       uint8 [n, >= longest proof]   row i holds proof_lens[i] bytes (a view whose rows lie further apart is taken as it is)
        proof_lens   [n], m [n]                    the used part of every row
        commitments  uint8 [n, m_stride, 32]       row i holds m[i] commitments
        min_values   uint64 [n, m_stride], min_present uint8 [n, m_stride], seed_nonces uint8 [n, 32], seed_present uint8 [n], or None
    Row slack is never read.  Holds the arrays alive; `.struct` can be passed to the *_mixed entry points any number of times."""

    def __init__(self, proofs, proof_lens, m, commitments, min_values=None, min_present=None, seed_nonces=None, label=b"", seed_present=None,
                 state=None, proof_stride=None):
        self.proof_lens, self.m, n = _mixed_meta(proof_lens, m)
        p = _host_array(proofs)
        if p.dtype != np.uint8 or p.ndim != 2 or p.shape[0] != n:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "proofs: a uint8 array of shape (n, row) expected")
        if not (n <= 1 or (p.strides[1] == 1 and p.strides[0] >= p.shape[1])):
            p = np.ascontiguousarray(p)
        self.proofs = p
        stride = int(proof_stride) if proof_stride is not None else (p.strides[0] if n > 1 else p.shape[1])
        commitments = np.ascontiguousarray(_host_array(commitments), dtype=np.uint8)
        if commitments.ndim != 3 or commitments.shape[0] != n or commitments.shape[2] != 32:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "commitments: an array of shape (n, m_stride, 32) expected")
        ms = commitments.shape[1]
        self.commitments = commitments
        self.min_values = None if min_values is None else _c(_host_array(min_values), np.uint64, (n, ms))
        self.min_present = None if min_present is None else _c(_host_array(min_present), np.uint8, (n, ms))
        self.seed_nonces = None if seed_nonces is None else _c(_host_array(seed_nonces), np.uint8, (n, 32))
        self.seed_present = None if seed_present is None else _c(_host_array(seed_present), np.uint8, (n,))
        self.label = np.frombuffer(bytes(label), dtype=np.uint8).copy() if len(label) else np.zeros(1, dtype=np.uint8)
        self.state = None if state is None else np.frombuffer(bytes(state), dtype=np.uint8).copy()
        self.n, self.m_stride = n, ms
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        self.struct = _lib.MixedBatch(n, ptr(self.proofs), stride, ptr(self.proof_lens), ptr(self.m), ms, ptr(self.commitments),
                                      ptr(self.min_values), ptr(self.min_present), ptr(self.seed_nonces), ptr(self.seed_present),
                                      ptr(self.state), ptr(self.label), len(label))


class DeviceMixedInput(DevicePackedInput):
    """MixedInput whose six row arrays already lie in DEVICE memory, for the *_mixed_device entry points: torch device tensors or
    (address, shape) pairs of the shapes given there (proofs may be a view whose rows lie further apart than they are long, or
    proof_stride= with an address; min_values any 8-byte dtype).  proof_lens and m are HOST arrays: they size the layout.  Ordering as
    for DevicePackedInput: order_before(engine) is called by verify_batch_mixed_device and ResidentBatch.from_mixed."""

    def __init__(self, proofs, proof_lens, m, commitments, min_values=None, min_present=None, seed_nonces=None, label=b"", seed_present=None,
                 state=None, proof_stride=None, item_states=None):
        self._keep, self.device_index, self._torch, self.synchronised = [], None, False, False
        self.proof_lens, self.m, n = _mixed_meta(proof_lens, m)
        addr_p, shape, stride = self._array(proofs, "proofs", 1, rows=True)
        if len(shape) != 2 or shape[0] != n:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "proofs: an array of shape (%d, row) expected, got %s" % (n, shape))
        stride = int(proof_stride) if proof_stride is not None else (stride if stride is not None else shape[1])
        addr_c, cshape, _ = self._array(commitments, "commitments", 1)
        if len(cshape) != 3 or cshape[0] != n or cshape[2] != 32:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "commitments: an array of shape (%d, m_stride, 32) expected, got %s" % (n, cshape))
        ms = cshape[1]

        def opt(a, name, itemsize, want):
            if a is None:
                return None
            addr, got, _ = self._array(a, name, itemsize)
            if got != want:
                raise api.ProofError(api.ProofErrorKind.InvalidLength, "%s: array of shape %s expected, got %s" % (name, want, got))
            return addr

        self.label = np.frombuffer(bytes(label), dtype=np.uint8).copy() if len(label) else np.zeros(1, dtype=np.uint8)
        self.state = None if state is None else np.frombuffer(bytes(state), dtype=np.uint8).copy()
        self.n, self.m_stride = n, ms
        self.struct = _lib.MixedBatch(n, addr_p, stride, self.proof_lens.ctypes.data, self.m.ctypes.data, ms, addr_c,
                                      opt(min_values, "min_values", 8, (n, ms)), opt(min_present, "min_present", 1, (n, ms)),
                                      opt(seed_nonces, "seed_nonces", 1, (n, 32)), opt(seed_present, "seed_present", 1, (n,)),
                                      None if self.state is None else self.state.ctypes.data, self.label.ctypes.data, len(label))
        self._item_states(item_states, n, opt)


def _verify_mixed(params, inp, action, chunk, device):
    eng, t = params.engine, int(params.extension_degree())
    masks = np.zeros((inp.n, t, 32), dtype=np.uint8)
    present = np.zeros(inp.n, dtype=np.uint8)
    err = ctypes.create_string_buffer(256)
    if device and getattr(inp, "item_states", None) is not None:
        # per-item transcripts have no blocking one-call form: the upload that takes them, then the resident verification
        batch = ResidentBatch.from_mixed(params, inp)
        try:
            got_masks, got_present = batch.verify_arrays(action, chunk)
            return got_masks.copy(), got_present.copy()
        finally:
            batch.close()
    if device:
        inp.order_before(eng)
    fn = eng.lib.bpp_verify_batch_mixed_device if device else eng.lib.bpp_verify_batch_mixed
    rc = fn(eng.ctx, params.handle, byref(inp.struct), int(action), chunk, masks.ctypes.data, present.ctypes.data, err, 256)
    api._check(rc, eng.ctx, err)
    return masks, present


def verify_batch_mixed(params, inp, action=api.VerifyAction.VerifyOnly, chunk=api.MAX_RANGE_PROOF_BATCH_SIZE):
    """RangeProof::verify_batch over a MixedInput in ONE C call (bpp_verify_batch_mixed): what the item form gives on the same rows.
    Returns (masks uint8 [n, t, 32], present uint8 [n])."""
    return _verify_mixed(params, inp, action, chunk, False)


def verify_batch_mixed_device(params, inp, action=api.VerifyAction.VerifyOnly, chunk=api.MAX_RANGE_PROOF_BATCH_SIZE):
    """verify_batch_mixed over a DeviceMixedInput (bpp_verify_batch_mixed_device): one kernel checks and packs the batch where it lies.
    Returns (masks uint8 [n, t, 32], present uint8 [n]) (host arrays)."""
    return _verify_mixed(params, inp, action, chunk, True)


class DeviceOpenings(DevicePackedInput):
    """The openings of a prove call whose arrays already lie in DEVICE memory + the bpp_prove_arrays that describes them, for
    bpp_prove_openings_device (include/bpp.h): no value, blinding factor, nonce or rng byte is copied to the host.  Torch device
    tensors or (address, shape) pairs:
        values       any 8-byte dtype [n, m_stride]     row i holds m[i] values
        blindings    uint8 [n, m_stride, t, 32]
        m            [n], a HOST array: it sizes the layout
        commitments  uint8 [n, m_stride, 32], or None: the engine makes them (bpp_prove_openings' rule)
        min_values   8-byte dtype [n, m_stride], min_present uint8 [n, m_stride], seed_nonces uint8 [n, 32], seed_present uint8 [n], or None
        rng_bytes    uint8 [n, rng_stride]              row i holds (rounds_i + 3) x 32 bytes
    Row slack is never read.  One transcript for the call: label= or state=.  Or one per item (bpp_prove_openings_device_transcripts):
    item_states= a uint8 [n, 203] device tensor (any byte address) or an (address, (n, 203)) pair, row i the STROBE state item i's
    proof continues; label and state are then not passed on.  Ordering as for DevicePackedInput."""

    def __init__(self, values, blindings, m, commitments=None, min_values=None, min_present=None, seed_nonces=None, seed_present=None,
                 rng_bytes=None, label=b"", state=None, item_states=None):
        self._keep, self.device_index, self._torch, self.synchronised = [], None, False, False
        self.m = np.ascontiguousarray(_host_array(m), dtype=np.uint32)
        if self.m.ndim != 1:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "m: an array of shape (n,) expected")
        n = self.m.shape[0]
        addr_v, vshape, _ = self._array(values, "values", 8)
        if len(vshape) != 2 or vshape[0] != n:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "values: an array of shape (%d, m_stride) expected, got %s" % (n, vshape))
        ms = vshape[1]
        addr_b, bshape, _ = self._array(blindings, "blindings", 1)
        if len(bshape) != 4 or bshape[:2] != (n, ms) or bshape[3] != 32:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "blindings: an array of shape (%d, %d, t, 32) expected, got %s" % (n, ms, bshape))
        addr_r, rshape, _ = self._array(rng_bytes, "rng_bytes", 1)
        if len(rshape) != 2 or rshape[0] != n:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "rng_bytes: an array of shape (%d, rng_stride) expected, got %s" % (n, rshape))

        def opt(a, name, itemsize, want):
            if a is None:
                return None
            addr, got, _ = self._array(a, name, itemsize)
            if got != want:
                raise api.ProofError(api.ProofErrorKind.InvalidLength, "%s: array of shape %s expected, got %s" % (name, want, got))
            return addr

        self.label = np.frombuffer(bytes(label), dtype=np.uint8).copy() if len(label) else np.zeros(1, dtype=np.uint8)
        self.label_bytes = bytes(label)
        self.state = None if state is None else np.frombuffer(bytes(state), dtype=np.uint8).copy()
        self.n, self.m_stride, self.t = n, ms, bshape[2]
        self.min_values, self.min_present, self.seed_nonces, self.seed_present = min_values, min_present, seed_nonces, seed_present
        self.struct = _lib.ProveArrays(n, self.m.ctypes.data, ms, addr_v, addr_b, opt(commitments, "commitments", 1, (n, ms, 32)),
                                       opt(min_values, "min_values", 8, (n, ms)), opt(min_present, "min_present", 1, (n, ms)),
                                       opt(seed_nonces, "seed_nonces", 1, (n, 32)), opt(seed_present, "seed_present", 1, (n,)), addr_r,
                                       rshape[1], None if self.state is None else self.state.ctypes.data, self.label.ctypes.data, len(label))
        self.item_states_rows = item_states
        self._item_states(item_states, n, opt)


class DeviceProved:
    """What prove_openings_device leaves: .commitments uint8 [n, 32 m_stride] and .proofs uint8 [n, longest proof] (device tensors;
    row i holds 32 m[i] and proof_lens[i] bytes, zero for a failed item), .status int32 [n, 2] (device: code, message id), and on the
    host .proof_lens, .m, .codes, the call's .rc and .message (the first failing item's).  .states (states=): uint8 [n, 203] on the
    device, row i the transcript item i's proof left advanced, zero for a failed item; else None."""

    def __init__(self, inp, commitments, proofs, proof_lens, status, codes, rc, message, states=None):
        self.inp, self.commitments, self.proofs, self.proof_lens, self.m = inp, commitments, proofs, proof_lens, inp.m
        self.status, self.codes, self.rc, self.message, self.states = status, codes, rc, message, states

    def as_mixed_input(self, label=None, state=None):
        """a DeviceMixedInput over the same tensors -- nothing is copied -- with the promises and nonces of the openings; label= / state=:
        the verifier's transcript (default: the prove call's -- for openings made with item_states=, the same starting rows, so that
        every output is verified under its own transcript where it lies)"""
        inp = self.inp
        if label is None and state is None and inp.item_states is not None:
            return DeviceMixedInput(self.proofs, self.proof_lens, self.m, self.commitments.view(self.commitments.shape[0], -1, 32),
                                    min_values=inp.min_values, min_present=inp.min_present, seed_nonces=inp.seed_nonces,
                                    seed_present=inp.seed_present, item_states=inp.item_states_rows)
        if label is None and state is None:
            label, state = inp.label_bytes, (None if inp.state is None else inp.state.tobytes())
        return DeviceMixedInput(self.proofs, self.proof_lens, self.m, self.commitments.view(self.commitments.shape[0], -1, 32),
                                min_values=inp.min_values, min_present=inp.min_present, seed_nonces=inp.seed_nonces,
                                label=b"" if label is None else label, seed_present=inp.seed_present, state=state)

    def messages(self, engine):
        """the message text of every item (bpp_prove_status_result over a host copy of .status)"""
        host = np.ascontiguousarray(self.status.cpu().numpy())
        out = []
        for i in range(host.shape[0]):
            r = _lib.ShardResult()
            api._check(engine.lib.bpp_prove_status_result(host[i:i + 1].ctypes.data_as(POINTER(_lib.DeviceProveStatus)), byref(r)), None)
            out.append((int(r.code), r.msg.decode()))
        return out


def prove_openings_device(params, inp, commitments_out=None, proofs_out=None, status_out=None, commit_stride=None, proof_stride=None,
                          states=None):
    """bpp_prove_openings over a DeviceOpenings (bpp_prove_openings_device): what bpp_prove_openings writes on host copies of the same
    arrays, with the proofs and commitments left in device memory.  A failed item never stops the others and does not raise: look at
    .codes / .rc / .message.  Raises when the whole call is refused or the engine faults.
    commitments_out / proofs_out / status_out: tensors (or (address, shape) pairs, with the strides) to write into; default: fresh ones.
    states (bpp_prove_openings_device_transcripts): True, or a uint8 [n, 203] device tensor (any byte address) or a raw device address
    -- the advanced transcripts come back as `.states`.  An `inp` made with item_states= goes through the same entry point."""
    import torch
    eng, t, n_bits = params.engine, int(params.extension_degree()), params.bit_length()
    n, ms = inp.n, inp.m_stride
    dev = torch.device("cuda", inp.device_index if inp.device_index is not None else int(eng.device))
    m_top = int(min(max(int(inp.m.max()), 1), ms)) if n else 1
    plen = 1 + 32 * (t + 5 + 2 * max((n_bits * m_top - 1).bit_length(), 0))
    if commitments_out is None:
        commitments_out = torch.zeros((n, 32 * ms), dtype=torch.uint8, device=dev)
    if proofs_out is None:
        proofs_out = torch.zeros((n, plen), dtype=torch.uint8, device=dev)
    if status_out is None:
        status_out = torch.zeros((n, 2), dtype=torch.int32, device=dev)

    def out(a, stride):
        if hasattr(a, "data_ptr"):
            return a.data_ptr(), int(stride if stride is not None else a.stride(0) * a.element_size())
        return int(a[0]), int(stride if stride is not None else a[1][1])

    addr_c, cstride = out(commitments_out, commit_stride)
    addr_p, pstride = out(proofs_out, proof_stride)
    addr_s = status_out.data_ptr() if hasattr(status_out, "data_ptr") else int(status_out[0])
    lens = np.zeros(n, dtype=np.uintp)
    unset = -(1 << 30)
    codes = np.full(n, unset, dtype=np.intc)
    err = ctypes.create_string_buffer(256)
    inp.order_before(eng)
    if states is False:
        states = None
    if states is None and inp.item_states is None:
        rc = eng.lib.bpp_prove_openings_device(eng.ctx, params.handle, byref(inp.struct), addr_c, cstride, addr_p, pstride,
                                               lens.ctypes.data_as(POINTER(c_size_t)), addr_s, codes.ctypes.data_as(POINTER(ctypes.c_int)), err, 256)
    else:
        if states is True:
            states = torch.zeros((n, 203), dtype=torch.uint8, device=dev)
        addr_t = None if states is None else ctypes.c_void_p(states.data_ptr() if hasattr(states, "data_ptr") else int(states))
        # (rows in: the call's label and state are not passed on; the engine refuses the combination)
        st = inp.struct if inp.item_states is None else inp.struct_without_transcript()
        rc = eng.lib.bpp_prove_openings_device_transcripts(eng.ctx, params.handle, byref(st), inp.item_states, addr_c, cstride, addr_p, pstride,
                                                           lens.ctypes.data_as(POINTER(c_size_t)), addr_t, addr_s,
                                                           codes.ctypes.data_as(POINTER(ctypes.c_int)), err, 256)
    if rc < 0 or (rc != 0 and (codes == unset).all()):
        api._check(rc, eng.ctx, err)
    return DeviceProved(inp, commitments_out, proofs_out, lens, status_out, codes, rc, err.value.decode(), states)


def prove_device_stats(engine):
    """bpp_prove_device_stats as a dict: calls, items, device_findings, host_findings"""
    s = _lib.ProveDeviceStats()
    api._check(engine.lib.bpp_prove_device_stats(engine.ctx, byref(s)), engine.ctx)
    return {k: int(getattr(s, k)) for k, _ in _lib.ProveDeviceStats._fields_}


PROVE_PLAN_ITEM_STATES = 1
PROVE_SUMMARY_WRITTEN = 1
PROVE_MSG_EMPTY = 17


class ProvePlan:
    """A resident prove plan (bpp_prove_plan_create): the shape of a prove call from device arrays -- m (a HOST array), the strides,
    which optional arrays every call brings, the call's one transcript (label= / state=) or item_states=True for one transcript
    row per item -- planned, carved and staged once.  enqueue() then proves a DeviceOpenings of that shape on the engine's stream
    without any host work of size n and without waiting (bpp_prove_enqueue).  `.proof_lens` and `.host_status` (the code of an item
    the host refuses from m alone, else 0) are known from here on.  close() waits for the plan's work and frees it."""

    def __init__(self, engine, params, m, m_stride=None, rng_stride=None, commitments=False, min_values=False, min_present=False,
                 seed_nonces=False, seed_present=False, label=b"", state=None, item_states=False, commit_stride=None, proof_stride=None):
        self.engine, self.params = engine, params
        self.m = np.ascontiguousarray(_host_array(m), dtype=np.uint32)
        n, t, n_bits = self.m.shape[0], int(params.extension_degree()), params.bit_length()
        m_top = max(int(self.m.max()), 1) if n else 1
        self.m_stride = int(m_stride) if m_stride is not None else m_top
        rounds_top = max((n_bits * min(m_top, self.m_stride) - 1).bit_length(), 0)
        self.rng_stride = int(rng_stride) if rng_stride is not None else 32 * (rounds_top + 3)
        self.commit_stride = int(commit_stride) if commit_stride is not None else 32 * self.m_stride
        self.proof_stride = int(proof_stride) if proof_stride is not None else 1 + 32 * (t + 5 + 2 * rounds_top)
        self.n, self.t, self.item_states = n, t, bool(item_states)
        self._label = np.frombuffer(bytes(label), dtype=np.uint8).copy() if len(label) else np.zeros(1, dtype=np.uint8)
        self._state = None if state is None else np.frombuffer(bytes(state), dtype=np.uint8).copy()
        self.label_bytes, self.state_bytes = bytes(label), (None if state is None else bytes(state))
        given = lambda flag: ctypes.c_void_p(1) if flag else None  # noqa: E731  (read for "will be given" alone)
        shape = _lib.ProveArrays(n, self.m.ctypes.data, self.m_stride, given(True), given(True), given(commitments), given(min_values),
                                 given(min_present), given(seed_nonces), given(seed_present), given(True), self.rng_stride,
                                 None if (self._state is None or item_states) else self._state.ctypes.data,
                                 None if item_states else self._label.ctypes.data, 0 if item_states else len(label))
        handle = c_uint64()
        err = ctypes.create_string_buffer(256)
        api._check(engine.lib.bpp_prove_plan_create(engine.ctx, params.handle, byref(shape), self.commit_stride, self.proof_stride,
                                                    PROVE_PLAN_ITEM_STATES if item_states else 0, byref(handle), err, 256), engine.ctx, err)
        self.handle = handle.value
        self.proof_lens = np.zeros(n, dtype=np.uintp)
        self.host_status = np.zeros(n, dtype=np.intc)
        api._check(engine.lib.bpp_prove_plan_shape(engine.ctx, self.handle, self.proof_lens.ctypes.data_as(POINTER(c_size_t)),
                                                   self.host_status.ctypes.data_as(POINTER(ctypes.c_int))), engine.ctx)

    def enqueue(self, openings, live=None, states=False, commitments_out=None, proofs_out=None, status_out=None, ok_mask=None,
                summary=None, shape_vector=False):
        """bpp_prove_enqueue over a DeviceOpenings of the plan's shape.  What wrote the arrays must be ordered before the engine's stream:
        an engine made on torch's current stream has that by construction and nothing is synchronised; otherwise torch's current
        stream is synchronised first (openings.order_before; with raw addresses the caller orders).  live: a contiguous uint8
        device tensor of n bytes (0 = dead: the item's rows are never read), or None.  states: True or a uint8 [n, 203] device tensor
        -- the advanced transcripts.  The outputs default to fresh tensors.  shape_vector=True passes the openings' m for the
        engine to compare with the plan's; the default passes none ("the plan's own").  Returns a ProveEnqueued."""
        import torch
        eng, n = self.engine, self.n
        dev = torch.device("cuda", int(eng.device))
        if commitments_out is None:
            commitments_out = torch.zeros((n, self.commit_stride), dtype=torch.uint8, device=dev)
        if proofs_out is None:
            proofs_out = torch.zeros((n, self.proof_stride), dtype=torch.uint8, device=dev)
        if status_out is None:
            status_out = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        if ok_mask is None:
            ok_mask = torch.zeros((n,), dtype=torch.uint8, device=dev)
        if summary is None:
            summary = torch.zeros((8,), dtype=torch.int32, device=dev)
        if states is True:
            states = torch.zeros((n, 203), dtype=torch.uint8, device=dev)
        elif states is False:
            states = None
        addr = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else int(a))  # noqa: E731
        st = openings.struct_without_transcript()
        if not shape_vector:
            st.m = None
        openings.order_before(eng)
        ticket = c_uint64()
        api._check(eng.lib.bpp_prove_enqueue(eng.ctx, self.handle, byref(st), openings.item_states, addr(live), addr(commitments_out),
                                             addr(proofs_out), addr(states), addr(status_out), addr(ok_mask), addr(summary), byref(ticket)),
                   eng.ctx)
        return ProveEnqueued(self, openings, ticket.value, commitments_out, proofs_out, status_out, ok_mask, summary, states, live)

    def close(self):
        if self.handle:
            self.engine.lib.bpp_prove_plan_destroy(self.engine.ctx, self.handle)
            self.handle = 0


class ProveEnqueued:
    """What ProvePlan.enqueue returns: `.proofs`, `.commitments`, `.status` (int32 [n, 2]: code, message id), `.ok_mask` (uint8 [n]),
    `.summary` (int32 [8]: code, message id, index, flags, n_ok, n_failed, n_empty, 0) and `.states` -- device tensors, valid in
    stream order behind the call -- and the ticket: done() is one event query, wait() blocks until the call has run, result() waits
    and returns the summary as a dict with the blocking call's code and text."""

    def __init__(self, plan, inp, ticket, commitments, proofs, status, ok_mask, summary, states, live):
        self.plan, self.inp, self.engine, self.ticket = plan, inp, plan.engine, ticket
        self.commitments, self.proofs, self.status, self.ok_mask, self.summary, self.states = commitments, proofs, status, ok_mask, summary, states
        self.live, self.proof_lens, self.m = live, plan.proof_lens, plan.m

    def done(self):
        d = ctypes.c_int()
        api._check(self.engine.lib.bpp_enqueue_done(self.engine.ctx, self.ticket, byref(d)), self.engine.ctx)
        return bool(d.value)

    def wait(self):
        api._check(self.engine.lib.bpp_enqueue_wait(self.engine.ctx, self.ticket), self.engine.ctx)

    def result(self):
        self.wait()
        host = np.ascontiguousarray(self.summary.cpu().numpy())
        r = _lib.ShardResult()
        api._check(self.engine.lib.bpp_prove_summary_result(host.ctypes.data_as(POINTER(_lib.DeviceProveSummary)), byref(r)), None)
        return {"code": r.code, "msg": r.msg.decode(errors="replace"), "msg_id": int(host[1]), "index": int(host[2]), "flags": int(host[3]),
                "n_ok": int(host[4]), "n_failed": int(host[5]), "n_empty": int(host[6])}

    def as_mixed_input(self):
        """a DeviceMixedInput over the output tensors -- nothing is copied -- under the transcripts the proofs were made under, with
        `.live` = the ok mask: ResidentBatch.refill takes it as the refill's live mask, so that a failed item never reaches the
        verifier as a parse finding"""
        if self.inp.item_states is not None:
            inp = DeviceProved.as_mixed_input(self)
        else:
            inp = DeviceProved.as_mixed_input(self, label=self.plan.label_bytes, state=self.plan.state_bytes)
        inp.live = self.ok_mask
        return inp


def prove_enqueue_stats(engine):
    """bpp_prove_enqueue_stats as a dict: calls, first_calls, host_waits, allocations"""
    s = _lib.ProveEnqueueStats()
    api._check(engine.lib.bpp_prove_enqueue_stats(engine.ctx, byref(s)), engine.ctx)
    return {k: int(getattr(s, k)) for k, _ in _lib.ProveEnqueueStats._fields_}


TOP_NEW, TOP_APPEND, TOP_CHALLENGE = 1, 2, 3  # BPP_TOP_* of include/bpp.h
TOP_MAX_OPS, TOP_LABEL_MAX, TOP_LEN_MAX, TOPS_WRITTEN = 8, 64, 65536, 1


class TNew:
    """Transcript::new(label) on every live row, whatever it held: only as the first operation of a program"""

    def __init__(self, label):
        self.label = bytes(label)


class TAppend:
    """append_message(label, row i of data).  data: a uint8 [n, len] device tensor (rows may be further apart than len: stride(0) >=
    len), or an (address, (n, len)) / (address, (n, len), stride) tuple.  lens: an int32 / uint32 [n] device tensor (or an address)
    of per-row lengths under the cap len, or None.  append_u64 is an append of eight little-endian bytes."""

    def __init__(self, label, data, lens=None):
        self.label, self.data, self.lens = bytes(label), data, lens


class TChallenge:
    """challenge_bytes(label, nbytes) into row i of out: a uint8 [n, nbytes] device tensor (stride(0) >= nbytes), a tuple as for
    TAppend, or None for a fresh tensor"""

    def __init__(self, label, nbytes, out=None):
        self.label, self.nbytes, self.out = bytes(label), int(nbytes), out


TOP_APPEND_POINT, TOP_CHALLENGE_SCALAR = 16, 17
TOP_RNG_BEGIN, TOP_RNG_REKEY, TOP_RNG_FINALIZE, TOP_RNG_FILL, TOP_RNG_FILL32, TOP_RNG_SCALARS = 32, 33, 34, 35, 36, 37
TOPS_IDENTITY, TOPS_ZERO_SCALAR = 2, 4


class TAppendPoint(TAppend):
    """validate_and_append_point(label, row i of data): data is a uint8 [n, 32] device tensor (or a tuple as for TAppend).  A row of 32
    zero bytes -- the identity's encoding -- makes its transcript row void (record flag TOPS_IDENTITY)."""

    def __init__(self, label, data):
        TAppend.__init__(self, label, data, None)


class TChallengeScalar(TChallenge):
    """challenge_scalar(label): 64 challenge bytes reduced wide mod l, the 32 canonical bytes into row i of out (uint8 [n, 32], a
    tuple, or None for a fresh tensor).  A zero scalar makes the row void (TOPS_ZERO_SCALAR)."""

    def __init__(self, label, out=None):
        TChallenge.__init__(self, label, 32, out)


class TRngBegin:
    """build_rng(): the program's transcript RNG becomes a clone of the row's transcript as it stands here.  The RNG lives for the
    length of the program; the row's 203 bytes are not changed by any TRng* operation."""
    label = b""


class TRngRekey(TAppend):
    """rekey_with_witness_bytes(label, row i of data): data and lens as for TAppend.  The rows are secrets."""


class TRngFinalize:
    """finalize(&mut rng): entropy is a uint8 [n, 32] device tensor (or tuple) -- the one draw from the caller's own RNG, per row -- or
    None for the reference's NullRng (32 zero bytes)"""
    label = b""

    def __init__(self, entropy=None):
        self.entropy = entropy


class TRngFill(TChallenge):
    """one fill_bytes(nbytes) of the finalised RNG into row i of out (as for TChallenge)"""

    def __init__(self, nbytes, out=None):
        TChallenge.__init__(self, b"", nbytes, out)


class TRngFill32(TRngFill):
    """nbytes / 32 successive fill_bytes(32): what a consumer drawing 32 bytes at a time sees -- the prover's rng row"""


class TRngScalars(TChallenge):
    """count successive Scalar::random(&mut rng), 32 canonical bytes each, into row i of out (uint8 [n, 32 * count]).  A zero scalar
    makes the row void (TOPS_ZERO_SCALAR); the call does not redraw."""

    def __init__(self, count, out=None):
        TChallenge.__init__(self, b"", 32 * int(count), out)


# (class, kind), the most derived first: what transcript_ops makes of an operation
_TOP_READS = [(TAppendPoint, TOP_APPEND_POINT), (TRngRekey, TOP_RNG_REKEY), (TAppend, TOP_APPEND)]
_TOP_WRITES = [(TChallengeScalar, TOP_CHALLENGE_SCALAR), (TRngFill32, TOP_RNG_FILL32), (TRngFill, TOP_RNG_FILL), (TRngScalars, TOP_RNG_SCALARS),
               (TChallenge, TOP_CHALLENGE)]


class TranscriptsEnqueued:
    """What transcript_ops returns: `.states` (the rows, advanced in place), `.outputs` (one tensor -- or whatever was passed -- per
    operation that writes rows: TChallenge, TChallengeScalar, TRngFill, TRngFill32, TRngScalars, in program order), `.done_mask` (uint8 [n]: 1 where the row was advanced) and `.record` (int32 [4]: n_done, n_void,
    first_void, flags) -- valid in stream order behind the call -- and the ticket: done() is one event query, wait() blocks until
    the call has run, result() waits and returns the record as a dict (first_void None where no row was void)."""

    def __init__(self, engine, ticket, states, outputs, done_mask, record, keep):
        self.engine, self.ticket, self.states, self.outputs, self.done_mask, self.record, self._keep = engine, ticket, states, outputs, done_mask, record, keep

    def done(self):
        d = ctypes.c_int()
        api._check(self.engine.lib.bpp_enqueue_done(self.engine.ctx, self.ticket, byref(d)), self.engine.ctx)
        return bool(d.value)

    def wait(self):
        api._check(self.engine.lib.bpp_enqueue_wait(self.engine.ctx, self.ticket), self.engine.ctx)

    def result(self):
        self.wait()
        host = [int(x) & 0xFFFFFFFF for x in self.record.cpu().numpy()]
        return {"n_done": host[0], "n_void": host[1], "first_void": None if host[2] == 0xFFFFFFFF else host[2], "flags": host[3]}


def transcript_ops(engine, states, ops, live=None, done_mask=None, record=None):
    """bpp_transcripts_enqueue: the program `ops` (TNew / TAppend / TChallenge; TAppendPoint / TChallengeScalar; TRngBegin / TRngRekey /
    TRngFinalize / TRngFill / TRngFill32 / TRngScalars -- at most 8) on the n rows of `states` -- a uint8 [n, 203]
    device tensor at any byte address (a slice of a larger tensor will do) or an (address, (n, 203)) pair -- in place, on the engine's
    stream, without waiting.  live: a uint8 [n] device tensor (0 = dead: the row is neither read nor written), or None.  done_mask and
    record default to fresh tensors.  Ordering is DevicePackedInput.order_before's: an engine made on torch's current stream needs
    nothing, otherwise torch's current stream is synchronised first (with raw addresses the caller orders).  Returns a
    TranscriptsEnqueued; a refused call raises ProofError with the field named."""
    import torch
    dev = torch.device("cuda", int(engine.device))
    order = DevicePackedInput.__new__(DevicePackedInput)
    order._keep, order.device_index, order._torch, order.synchronised = [], None, False, False

    def rows(a, name, width=None):
        """-> (address, n, width, stride)"""
        if isinstance(a, tuple) and len(a) == 3:
            return int(a[0]), int(a[1][0]), int(a[1][1]), int(a[2])
        addr, shape, stride = order._array(a, name, 1, rows=True)
        if len(shape) != 2 or (width is not None and shape[1] != width):
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "%s: an array of shape (n, %s) expected, got %s" % (name, width or "len", shape))
        return addr, shape[0], shape[1], (stride if stride is not None else shape[1])

    addr_s, n, _, stride_s = rows(states, "states", 203)
    if stride_s != 203:
        raise api.ProofError(api.ProofErrorKind.InvalidArgument, "states: rows of 203 bytes back to back expected")

    def flat(a, name, itemsize):
        if a is None:
            return None
        if not hasattr(a, "data_ptr"):
            return int(a)
        if a.element_size() != itemsize or not a.is_contiguous() or a.numel() != n:
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "%s: %d contiguous elements of %d bytes expected" % (name, n, itemsize))
        order._keep.append(a)
        order._torch = True
        return a.data_ptr()

    arr = (_lib.TranscriptOp * max(len(ops), 1))()
    labels, outputs = [], []
    for j, op in enumerate(ops[:len(arr)]):
        lab = np.frombuffer(op.label, dtype=np.uint8).copy() if len(op.label) else None
        labels.append(lab)
        o = arr[j]
        o.label, o.label_len = (None if lab is None else lab.ctypes.data), len(op.label)
        if isinstance(op, TNew):
            o.kind = TOP_NEW
        elif isinstance(op, TRngBegin):
            o.kind = TOP_RNG_BEGIN
        elif isinstance(op, TRngFinalize):
            o.kind = TOP_RNG_FINALIZE
            if op.entropy is not None:
                o.data_dev, rows_n, o.len, o.stride = rows(op.entropy, "ops[%d].entropy" % j)
                if rows_n != n:
                    raise api.ProofError(api.ProofErrorKind.InvalidLength, "ops[%d].entropy: %d rows for %d states" % (j, rows_n, n))
        elif isinstance(op, TAppend):
            o.kind = next(k for c, k in _TOP_READS if isinstance(op, c))
            if op.data is not None:
                o.data_dev, rows_n, o.len, o.stride = rows(op.data, "ops[%d].data" % j)
                if rows_n != n:
                    raise api.ProofError(api.ProofErrorKind.InvalidLength, "ops[%d].data: %d rows for %d states" % (j, rows_n, n))
            o.lens_dev = flat(op.lens, "ops[%d].lens" % j, 4)
        elif isinstance(op, TChallenge):
            o.kind = next(k for c, k in _TOP_WRITES if isinstance(op, c))
            out = op.out
            if out is None and op.nbytes:
                out = torch.zeros((n, op.nbytes), dtype=torch.uint8, device=dev)
            if out is not None:
                o.data_dev, rows_n, o.len, o.stride = rows(out, "ops[%d].out" % j, None if isinstance(out, tuple) else op.nbytes)
                if rows_n != n or o.len != op.nbytes:
                    raise api.ProofError(api.ProofErrorKind.InvalidLength, "ops[%d].out: (%d, %d) expected" % (j, n, op.nbytes))
            outputs.append(out)
        else:
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "ops[%d]: a T* operation of this module expected" % j)
    if done_mask is None:
        done_mask = torch.zeros((n,), dtype=torch.uint8, device=dev)
    if record is None:
        record = torch.zeros((4,), dtype=torch.int32, device=dev)
    addr_live, addr_done = flat(live, "live", 1), flat(done_mask, "done_mask", 1)
    addr_rec = record.data_ptr() if hasattr(record, "data_ptr") else int(record)
    order.order_before(engine)
    ticket = c_uint64()
    api._check(engine.lib.bpp_transcripts_enqueue(engine.ctx, ctypes.c_void_p(addr_s), n, arr, len(ops), addr_live, addr_done, addr_rec,
                                                  byref(ticket)), engine.ctx)
    return TranscriptsEnqueued(engine, ticket.value, states, outputs, done_mask, record, (order._keep, labels, arr))


def transcripts_stats(engine):
    """bpp_transcripts_stats as a dict: calls, first_calls, host_waits"""
    s = _lib.TranscriptsStats()
    api._check(engine.lib.bpp_transcripts_stats(engine.ctx, byref(s)), engine.ctx)
    return {k: int(getattr(s, k)) for k, _ in _lib.TranscriptsStats._fields_}


ROWS_K_MAX, ROWS_WRITTEN, ROWS_SCALAR, ROWS_POINT = 16, 1, 2, 4  # BPP_ROWS_* of include/bpp.h


class RowsEnqueued(TranscriptsEnqueued):
    """What rows_msm and rows_scalar_muladd return: `.out` (uint8 [n, 32], or whatever was passed), `.done_mask` (uint8 [n]: 1 where the
    row was written) and `.record` (int32 [4]: n_done, n_void, first_void, flags -- ROWS_WRITTEN | ROWS_SCALAR | ROWS_POINT) -- valid in
    stream order behind the call -- and the ticket: done(), wait(), result() as for TranscriptsEnqueued."""

    def __init__(self, engine, ticket, out, done_mask, record, keep):
        TranscriptsEnqueued.__init__(self, engine, ticket, None, [out], done_mask, record, keep)
        self.out = out


class _RowArrays:
    """the row arrays of one bpp_rows_*_enqueue: addresses, shapes and the ordering of DevicePackedInput"""

    def __init__(self, engine):
        import torch
        self.engine, self.torch, self.dev = engine, torch, torch.device("cuda", int(engine.device))
        self.order = DevicePackedInput.__new__(DevicePackedInput)
        self.order._keep, self.order.device_index, self.order._torch, self.order.synchronised = [], None, False, False

    def rows(self, a, name):
        """a uint8 [rows, width] device tensor (stride(0) >= width) or an (address, (rows, width)[, stride]) tuple
        -> (address, rows, width, stride)"""
        if isinstance(a, tuple) and len(a) == 3:
            return int(a[0]), int(a[1][0]), int(a[1][1]), int(a[2])
        addr, shape, stride = self.order._array(a, name, 1, rows=True)
        if len(shape) != 2:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "%s: an array of shape (n, len) expected, got %s" % (name, shape))
        return addr, shape[0], shape[1], (stride if stride is not None else shape[1])

    def flat(self, a, name, n):
        if a is None:
            return None
        if not hasattr(a, "data_ptr"):
            return int(a)
        if a.element_size() != 1 or not a.is_contiguous() or a.numel() != n:
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "%s: %d contiguous bytes expected" % (name, n))
        self.order._keep.append(a)
        self.order._torch = True
        return a.data_ptr()

    def outputs(self, n, out, done_mask, record):
        """-> (out, its address, its stride, done_mask, its address, record, its address), fresh tensors where None"""
        torch = self.torch
        if out is None:
            out = torch.zeros((n, 32), dtype=torch.uint8, device=self.dev)
        addr_o, rows_o, width_o, stride_o = self.rows(out, "out")
        if rows_o != n or width_o != 32:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "out: (%d, 32) expected" % n)
        if done_mask is None:
            done_mask = torch.zeros((n,), dtype=torch.uint8, device=self.dev)
        if record is None:
            record = torch.zeros((4,), dtype=torch.int32, device=self.dev)
        addr_rec = record.data_ptr() if hasattr(record, "data_ptr") else int(record)
        return out, addr_o, stride_o, done_mask, self.flat(done_mask, "done_mask", n), record, addr_rec


def rows_msm(engine, scalars, points, K, out=None, live=None, done_mask=None, record=None):
    """bpp_rows_msm_enqueue: out[i] = sum_{k < K} scalars[i][k] * points[i][k], constant-time in the scalars, on the engine's stream,
    without waiting.  scalars: a uint8 [n, 32 K] device tensor at any byte address (stride(0) >= 32 K) or an (address, (n, 32 K),
    stride) tuple -- SECRETS, read where they lie.  points: likewise [n, 32 K], or a tensor of shape [K, 32]: ONE row of K bases shared
    by every row.  out: uint8 [n, 32] (stride(0) >= 32), a tuple, or None for a fresh tensor.  live: uint8 [n] (0 = dead: nothing of the
    row is read, its output is zeroed), or None.  A live row with a scalar >= l or a point that does not decode is VOID: zero output,
    done_mask 0, ROWS_SCALAR / ROWS_POINT in the record.  Ordering as for transcript_ops.  Returns a RowsEnqueued; a refused call raises
    ProofError with the field named."""
    ra = _RowArrays(engine)
    K = int(K)
    addr_s, n, width_s, stride_s = ra.rows(scalars, "scalars")
    if width_s != 32 * K:
        raise api.ProofError(api.ProofErrorKind.InvalidLength, "scalars: rows of 32 K = %d bytes expected, got %d" % (32 * K, width_s))
    addr_p, rows_p, width_p, stride_p = ra.rows(points, "points")
    if width_p == 32 and rows_p == K and (K > 1 or n != 1):
        stride_p = 0  # shared bases
    elif rows_p != n or width_p != 32 * K:
        raise api.ProofError(api.ProofErrorKind.InvalidLength, "points: (%d, %d) or (%d, 32) expected, got (%d, %d)" % (n, 32 * K, K, rows_p, width_p))
    out, addr_o, stride_o, done_mask, addr_done, record, addr_rec = ra.outputs(n, out, done_mask, record)
    addr_live = ra.flat(live, "live", n)
    desc = _lib.RowsMsm(n, K, addr_s, stride_s, addr_p, stride_p)
    ra.order.order_before(engine)
    ticket = c_uint64()
    api._check(engine.lib.bpp_rows_msm_enqueue(engine.ctx, byref(desc), addr_o, stride_o, addr_live, addr_done, addr_rec, byref(ticket)), engine.ctx)
    return RowsEnqueued(engine, ticket.value, out, done_mask, record, (ra.order._keep, desc))


def rows_scalar_muladd(engine, a, b, c=None, out=None, live=None, done_mask=None, record=None):
    """bpp_rows_scalar_enqueue: out[i] = a[i] * b[i] + c[i] mod l, 32 canonical little-endian bytes per row, on the engine's stream,
    without waiting.  a, b, c: uint8 [n, 32] device tensors at any byte address (stride(0) >= 32), (address, (n, 32), stride) tuples,
    or a tensor of shape [32] / [1, 32]: one scalar for every row; c None adds nothing.  At least one operand must give n (or pass
    out).  A non-canonical operand voids the row (ROWS_SCALAR).  out, live, done_mask, record, ordering and the return value as for
    rows_msm."""
    ra = _RowArrays(engine)
    ops, n = [], None
    for name, x in (("a", a), ("b", b), ("c", c)):
        if x is None:
            if name != "c":
                raise api.ProofError(api.ProofErrorKind.InvalidArgument, "%s: an operand expected" % name)
            ops.append(None)
            continue
        if hasattr(x, "dim") and x.dim() == 1:
            x = x.reshape(1, -1)
        addr, rows_x, width, stride = ra.rows(x, name)
        if width != 32:
            raise api.ProofError(api.ProofErrorKind.InvalidLength, "%s: rows of 32 bytes expected, got %d" % (name, width))
        broadcast = rows_x == 1 and not (isinstance(x, tuple) and stride)
        if not broadcast:
            if n is not None and rows_x != n:
                raise api.ProofError(api.ProofErrorKind.InvalidLength, "%s: %d rows, another operand has %d" % (name, rows_x, n))
            n = rows_x
        ops.append(_lib.ScalarRows(addr, 0 if broadcast else stride))
    if n is None:
        n = 1 if out is None else ra.rows(out, "out")[1]
    out, addr_o, stride_o, done_mask, addr_done, record, addr_rec = ra.outputs(n, out, done_mask, record)
    addr_live = ra.flat(live, "live", n)
    ra.order.order_before(engine)
    ticket = c_uint64()
    api._check(engine.lib.bpp_rows_scalar_enqueue(engine.ctx, n, byref(ops[0]), byref(ops[1]), None if ops[2] is None else byref(ops[2]), addr_o,
                                                  stride_o, addr_live, addr_done, addr_rec, byref(ticket)), engine.ctx)
    return RowsEnqueued(engine, ticket.value, out, done_mask, record, (ra.order._keep, ops))


def rows_stats(engine):
    """bpp_rows_stats as a dict: calls, first_calls, host_waits"""
    s = _lib.RowsStats()
    api._check(engine.lib.bpp_rows_stats(engine.ctx, byref(s)), engine.ctx)
    return {k: int(getattr(s, k)) for k, _ in _lib.RowsStats._fields_}


def device_pointer_kind(engine, address):
    """bpp_device_pointer_check: 0 this engine's device memory, 1 another device's, 2 host or unknown, 3 managed (launches nothing)"""
    kind = ctypes.c_int(-1)
    api._check(engine.lib.bpp_device_pointer_check(engine.ctx, ctypes.c_void_p(int(address)), byref(kind)), engine.ctx)
    return kind.value


def ingest_stats(engine):
    """bpp_ingest_stats -> (device_calls, host_fallback_calls, fallback_bytes) of the engine's uploads from device memory"""
    s = _lib.IngestStats()
    api._check(engine.lib.bpp_ingest_stats(engine.ctx, byref(s)), engine.ctx)
    return int(s.device_calls), int(s.host_fallback_calls), int(s.fallback_bytes)


class Batcher:
    """bpp_batcher: many host threads, each calling verify(inp) with ONE reference batch; the calls that are waiting are pooled
    into grouped engine calls (bpp_verify_resident_groups), every caller gets the outcome of a call of its own.  `shape`: a
    PackedInput whose proof length, aggregation factor and label say what can be pooled."""

    def __init__(self, params, shape, lanes=0, max_wait_us=0, max_calls=64):
        self.params, self.engine = params, params.engine
        self.handle = ctypes.c_void_p()
        api._check(self.engine.lib.bpp_batcher_create(self.engine.ctx, params.handle, byref(shape.struct), lanes, max_wait_us, max_calls,
                                                      byref(self.handle)), self.engine.ctx)

    def verify(self, inp):
        """blocks; raises ProofError exactly as verify_batch(params, inp, VerifyOnly, chunk=0) would"""
        err = ctypes.create_string_buffer(256)
        api._check(self.engine.lib.bpp_batcher_verify(self.handle, byref(inp.struct), err, 256), None, err)

    def verify_action(self, inp, action):
        """any VerifyAction through the pool: returns (masks uint8 [n, t, 32], present uint8 [n]) exactly as
        verify_batch(params, inp, action, chunk=0) would, or raises its ProofError"""
        t = int(self.params.extension_degree())
        masks = np.zeros((inp.n, t, 32), dtype=np.uint8)
        present = np.zeros(inp.n, dtype=np.uint8)
        err = ctypes.create_string_buffer(256)
        api._check(self.engine.lib.bpp_batcher_verify_action(self.handle, byref(inp.struct), int(action), masks.ctypes.data,
                                                             present.ctypes.data, err, 256), None, err)
        return masks, present

    def largest_pool(self):
        c, p = ctypes.c_uint32(), ctypes.c_uint32()
        self.engine.lib.bpp_batcher_largest_pool(self.handle, byref(c), byref(p))
        return c.value, p.value

    def set_limits(self, max_calls=0, max_proofs=0):
        api._check(self.engine.lib.bpp_batcher_set_limits(self.handle, max_calls, max_proofs), None)

    def stats(self):
        v = [c_uint64() for _ in range(3)]
        self.engine.lib.bpp_batcher_stats(self.handle, *[byref(x) for x in v])
        return dict(zip(("pooled_calls", "engine_calls", "solo_calls"), [x.value for x in v]))

    def verify_joint_stats(self):
        """bpp_batcher_verify_joint_stats: the joint final checks ("verify_joint" = 1) of the batcher's lanes, summed"""
        s = _lib.VerifyJointStats()
        api._check(self.engine.lib.bpp_batcher_verify_joint_stats(self.handle, byref(s)), None)
        return {n: int(getattr(s, n)) for n, _ in _lib.VerifyJointStats._fields_}

    def close(self):
        if self.handle:
            self.engine.lib.bpp_batcher_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class ProvePool:
    """bpp_prove_pool: many host threads, each calling prove(...) with a few proofs of any aggregation factors; the calls that are
    waiting are proved as ONE bpp_prove_batch_mixed on one of `lanes` contexts, every caller gets what a bpp_prove_batch_mixed
    of its own items would have returned.  The engine's prover options at creation hold on every lane."""

    STRIDE = 1 + 32 * (6 + 5 + 2 * 12)  # the longest proof any parameters make

    def __init__(self, params, lanes=0, max_wait_us=0, max_calls=64):
        self.params, self.engine = params, params.engine
        self.handle = ctypes.c_void_p()
        api._check(self.engine.lib.bpp_prove_pool_create(self.engine.ctx, params.handle, lanes, max_wait_us, max_calls,
                                                         byref(self.handle)), self.engine.ctx)

    @staticmethod
    def marshal(transcripts, statements, witnesses, rng_bytes):
        """the bpp_prove_item array of a call (api.RangeProof's marshalling: its host checks raise here), reusable"""
        return api.RangeProof._prove_marshal(transcripts, statements, witnesses, rng_bytes)

    def prove_marshalled(self, marshalled):
        """blocks; returns the proofs' bytes, or raises the ProofError of the call's first failing item"""
        _params, items, n, _keep = marshalled
        out = (ctypes.c_uint8 * (self.STRIDE * n))()
        lens = (c_size_t * n)()
        err = ctypes.create_string_buffer(256)
        api._check(self.engine.lib.bpp_prove_pool_prove(self.handle, items, n, out, self.STRIDE, lens, err, 256), None, err)
        raw = bytes(out)
        return [raw[i * self.STRIDE:i * self.STRIDE + lens[i]] for i in range(n)]

    def prove(self, transcripts, statements, witnesses, rng_bytes):
        """n x RangeProof::prove_with_rng (any aggregation factors) through the pool -> list of proof bytes"""
        return self.prove_marshalled(self.marshal(transcripts, statements, witnesses, rng_bytes))

    def prove_openings_marshalled(self, marshalled):
        """bpp_prove_pool_openings over api.RangeProof._openings_marshal's items; blocks; returns (commitments per item, proof
        bytes per item), or raises the ProofError of the call's first failing item"""
        _params, items, n, _keep = marshalled
        cstride = 32 * max(items[i].m for i in range(n))
        comms = (ctypes.c_uint8 * (cstride * n))()
        out = (ctypes.c_uint8 * (self.STRIDE * n))()
        lens = (c_size_t * n)()
        err = ctypes.create_string_buffer(256)
        api._check(self.engine.lib.bpp_prove_pool_openings(self.handle, items, n, comms, cstride, out, self.STRIDE, lens, err, 256), None, err)
        raw, craw = bytes(out), bytes(comms)
        return ([[craw[i * cstride + 32 * j:i * cstride + 32 * j + 32] for j in range(items[i].m)] for i in range(n)],
                [raw[i * self.STRIDE:i * self.STRIDE + lens[i]] for i in range(n)])

    def prove_openings(self, transcripts, witnesses, minimum_value_promises, seed_nonces, rng_bytes):
        """api.RangeProof.prove_openings through the pool -> (statements, list of proof bytes); raises the first failing item's error"""
        comms, proofs = self.prove_openings_marshalled(api.RangeProof._openings_marshal(transcripts, witnesses, minimum_value_promises,
                                                                                       seed_nonces, rng_bytes, self.params))
        sts = [api.RangeStatement.init(self.params, c, list(mins), sn) for c, mins, sn in zip(comms, minimum_value_promises, seed_nonces)]
        return sts, proofs

    def openings_stats(self):
        """bpp_prove_pool_openings_stats: requests of the openings kind, pooled engine calls that held requests of both kinds"""
        a, b = c_uint64(), c_uint64()
        api._check(self.engine.lib.bpp_prove_pool_openings_stats(self.handle, byref(a), byref(b)), None)
        return {"openings_calls": int(a.value), "both_kinds_calls": int(b.value)}

    def set_limits(self, max_calls=0, max_proofs=0):
        api._check(self.engine.lib.bpp_prove_pool_set_limits(self.handle, max_calls, max_proofs), None)

    def stats(self):
        v = [c_uint64() for _ in range(3)] + [ctypes.c_uint32() for _ in range(2)]
        self.engine.lib.bpp_prove_pool_stats(self.handle, *[byref(x) for x in v])
        return dict(zip(("pooled_calls", "engine_calls", "solo_calls", "largest_calls", "largest_proofs"), [x.value for x in v]))

    def check_stats(self):
        """bpp_prove_pool_check_stats: the self-check counters of every lane, summed (Engine.prove_check_stats); the first lane is
        the engine the pool was made from"""
        s = _lib.ProveCheckStats()
        api._check(self.engine.lib.bpp_prove_pool_check_stats(self.handle, byref(s)), None)
        return {n: int(getattr(s, n)) for n, _ in _lib.ProveCheckStats._fields_}

    def check_recovery_stats(self):
        """bpp_prove_pool_check_recovery_stats: Engine.prove_check_recovery_stats summed over the lanes"""
        replayed, mismatched = c_uint64(), c_uint64()
        api._check(self.engine.lib.bpp_prove_pool_check_recovery_stats(self.handle, byref(replayed), byref(mismatched)), None)
        return {"replayed": int(replayed.value), "mismatched": int(mismatched.value)}

    def close(self):
        if self.handle:
            self.engine.lib.bpp_prove_pool_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class ProvePipeline:
    """bpp_prove_submit / bpp_prove_collect on one engine: prove calls in flight from ONE thread.  submit(...) /
    submit_openings(...) take what RangeProof.prove_batch_mixed / RangeProof.prove_openings take and return a ticket at once (the
    engine has its own copy of the items by then); collect(ticket) blocks and returns what those calls return -- one RangeProof or
    ProofError per item -- and raises what they raise.  Tickets may be collected in any order.  `depth` lanes (1..8), each a
    context with the engine's prover options as they are at the first submit; the depth can only be set before the first submit
    of the engine (depth=None keeps what the engine has)."""

    STRIDE = ProvePool.STRIDE

    def __init__(self, params, depth=3):
        self.params, self.engine = params, params.engine
        if depth is not None:
            api._check(self.engine.lib.bpp_prove_pipeline_depth(self.engine.ctx, int(depth)), self.engine.ctx)
        self._jobs = {}  # ticket -> what collect needs: the engine's ticket (None: no item reached the engine), the marshalled items, ...
        self._next = 1

    def _submit(self, marshalled, openings, cstride):
        _p, items, n, _keep = marshalled
        ticket = c_uint64()
        err = ctypes.create_string_buffer(256)
        api._check(self.engine.lib.bpp_prove_submit(self.engine.ctx, self.params.handle, items, n, self.STRIDE, 1 if openings else 0, cstride,
                                                    byref(ticket), err, 256), None, err)
        return ticket.value

    def _ticket(self, job):
        t = self._next
        self._next += 1
        self._jobs[t] = job
        return t

    def submit(self, transcripts, statements, witnesses, rng_bytes):
        """RangeProof.prove_batch_mixed, submitted: returns a ticket"""
        if not statements or len(statements) != len(witnesses) or len(transcripts) != len(statements) or \
                len(rng_bytes) != len(statements):
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "Range statements, witnesses, transcripts length mismatch")
        res, keep = [None] * len(statements), []
        for i, (tr, st, w, rb) in enumerate(zip(transcripts, statements, witnesses, rng_bytes)):
            try:
                api.RangeProof._prove_marshal([tr], [st], [w], [rb])
                keep.append(i)
            except api.ProofError as e:
                res[i] = e
        job = {"openings": False, "res": res, "keep": keep, "engine_ticket": None}
        if keep:
            pick = lambda a: [a[i] for i in keep]  # noqa: E731
            job["marshalled"] = api.RangeProof._prove_marshal(pick(transcripts), pick(statements), pick(witnesses), pick(rng_bytes))
            job["engine_ticket"] = self._submit(job["marshalled"], False, 0)
        return self._ticket(job)

    def submit_openings(self, transcripts, witnesses, minimum_value_promises, seed_nonces, rng_bytes):
        """RangeProof.prove_openings (on this pipeline's parameters), submitted: returns a ticket"""
        n = len(witnesses)
        res, keep = [None] * n, []
        for i in range(n):
            try:
                api.RangeProof._openings_marshal([transcripts[i]], [witnesses[i]], [minimum_value_promises[i]], [seed_nonces[i]],
                                                 [rng_bytes[i]], self.params)
                keep.append(i)
            except api.ProofError as e:
                res[i] = e
        job = {"openings": True, "res": res, "keep": keep, "engine_ticket": None, "witnesses": [witnesses[i] for i in keep],
               "promises": [list(minimum_value_promises[i]) for i in keep], "nonces": [seed_nonces[i] for i in keep]}
        if keep:
            pick = lambda a: [a[i] for i in keep]  # noqa: E731
            job["marshalled"] = api.RangeProof._openings_marshal(pick(transcripts), pick(witnesses), pick(minimum_value_promises),
                                                                 pick(seed_nonces), pick(rng_bytes), self.params)
            job["cstride"] = 32 * max(len(w.openings) for w in job["witnesses"])
            job["engine_ticket"] = self._submit(job["marshalled"], True, job["cstride"])
        return self._ticket(job)

    def done(self, ticket):
        """True once collect(ticket) would not wait; never blocks"""
        job = self._jobs[ticket]
        if job["engine_ticket"] is None:
            return True
        d = ctypes.c_int()
        api._check(self.engine.lib.bpp_prove_ticket_done(self.engine.ctx, job["engine_ticket"], byref(d)), None)
        return bool(d.value)

    def collect(self, ticket):
        """blocks until the ticket's call is done: the list RangeProof.prove_batch_mixed returns, or for a ticket of
        submit_openings the (statements, proofs) pair RangeProof.prove_openings returns"""
        job = self._jobs.pop(ticket)
        res, keep, openings = job["res"], job["keep"], job["openings"]
        sts = list(res)
        if not keep:
            return (sts, res) if openings else res
        eng, params = self.engine, self.params
        _p, items, n, _keep = job["marshalled"]
        stride, cstride = self.STRIDE, job.get("cstride", 0)
        out = (ctypes.c_uint8 * (stride * n))()
        comms = (ctypes.c_uint8 * (cstride * n))() if openings else None
        lens = (c_size_t * n)()
        status = (ctypes.c_int * n)()
        err = ctypes.create_string_buffer(256)
        rc = eng.lib.bpp_prove_collect(eng.ctx, job["engine_ticket"], comms, out, lens, status, err, 256)
        codes = [status[k] for k in range(n)]
        faults = [c for c in [rc] + codes if c < 0 and c != api.EngineError.SELF_CHECK]
        if faults:
            api._check(min(faults), None, err)
        raw, craw = bytes(out), bytes(comms) if openings else b""
        for k, i in enumerate(keep):
            if codes[k] == 0:
                res[i] = api.RangeProof.from_bytes(raw[k * stride:k * stride + lens[k]])
                if openings:
                    cs = [craw[k * cstride + 32 * j:k * cstride + 32 * j + 32] for j in range(items[k].m)]
                    sts[i] = api.RangeStatement.init(params, cs, job["promises"][k], job["nonces"][k])
                continue
            # (the parent context holds this ticket's note of failed mask-recovery replays since the collect)
            if openings:
                first = None
                if codes[k] == api.EngineError.SELF_CHECK and job["nonces"][k] is not None:
                    o = job["witnesses"][k].openings[0]
                    first = api._buf(params.commit(o.v, o.r))
                eng.lib.bpp_prove_openings_item_message(eng.ctx, params.handle, byref(items[k]), first, cstride, stride, codes[k], err, 256)
            else:
                eng.lib.bpp_prove_item_message(eng.ctx, params.handle, byref(items[k]), stride, codes[k], err, 256)
            msg = err.value.decode(errors="replace")
            if codes[k] == api.EngineError.SELF_CHECK:
                res[i] = sts[i] = api.EngineError("bpp engine error %d: %s" % (codes[k], msg), codes[k])
            else:
                res[i] = sts[i] = api.ProofError(codes[k], msg)
        return (sts, res) if openings else res

    def close(self):
        """collects and drops whatever is still outstanding (the lanes live as long as the engine does)"""
        for t in list(self._jobs):
            try:
                self.collect(t)
            except (api.ProofError, api.EngineError):
                pass


def verify_groups_actions(rb, bounds, actions):
    """bpp_verify_resident_groups_actions: one VerifyAction per group -> (result dicts, masks [n, t, 32], present [n])"""
    G = len(bounds) - 1
    arr = (ctypes.c_uint32 * (G + 1))(*bounds)
    act = (ctypes.c_int * G)(*[int(a) for a in actions])
    out = (_lib.ShardResult * G)()
    masks = np.zeros((rb.n, rb.t, 32), dtype=np.uint8)
    present = np.zeros(rb.n, dtype=np.uint8)
    api._check(rb.engine.lib.bpp_verify_resident_groups_actions(rb.engine.ctx, rb.handle, arr, G, act, out, masks.ctypes.data,
                                                                present.ctypes.data), rb.engine.ctx)
    return [{"code": r.code, "tier": r.tier, "index": r.index, "msg": r.msg.decode(errors="replace")} for r in out], masks, present


def runtime_info(engine):
    """bpp_runtime_info_get as a dict"""
    info = _lib.RuntimeInfo()
    api._check(engine.lib.bpp_runtime_info_get(engine.ctx, byref(info)), engine.ctx)
    return {n: getattr(info, n) for n, _ in _lib.RuntimeInfo._fields_}


def verify_groups(rb, bounds):
    """bpp_verify_resident_groups on a resident batch: group g = proofs [bounds[g], bounds[g+1]) -> list of result dicts"""
    G = len(bounds) - 1
    arr = (ctypes.c_uint32 * (G + 1))(*bounds)
    out = (_lib.ShardResult * G)()
    api._check(rb.engine.lib.bpp_verify_resident_groups(rb.engine.ctx, rb.handle, arr, G, out), rb.engine.ctx)
    return [{"code": r.code, "tier": r.tier, "index": r.index, "msg": r.msg.decode(errors="replace")} for r in out]


class Pipeline:
    """bpp_verify_submit_packed / bpp_verify_collect on one engine: upload k+1 overlaps verify k inside ONE context"""

    def __init__(self, params, depth=None):
        self.params, self.engine, self.t = params, params.engine, int(params.extension_degree())
        if depth is not None:
            api._check(self.engine.lib.bpp_ctx_pipeline_depth(self.engine.ctx, int(depth)), self.engine.ctx)
        self._n = {}

    def submit(self, inp, action=api.VerifyAction.VerifyOnly, chunk=api.MAX_RANGE_PROOF_BATCH_SIZE):
        ticket = c_uint64()
        err = ctypes.create_string_buffer(256)
        rc = self.engine.lib.bpp_verify_submit_packed(self.engine.ctx, self.params.handle, byref(inp.struct), int(action), chunk,
                                                      byref(ticket), err, 256)
        api._check(rc, None, err)
        self._n[ticket.value] = (inp.n, int(action))
        return ticket.value

    def collect(self, ticket):
        n, action = self._n.pop(ticket)
        err = ctypes.create_string_buffer(256)
        if action == int(api.VerifyAction.VerifyOnly):
            api._check(self.engine.lib.bpp_verify_collect(self.engine.ctx, ticket, None, None, err, 256), None, err)
            return None, None
        masks = np.zeros((n, self.t, 32), dtype=np.uint8)
        present = np.zeros(n, dtype=np.uint8)
        api._check(self.engine.lib.bpp_verify_collect(self.engine.ctx, ticket, masks.ctypes.data, present.ctypes.data, err, 256),
                   None, err)
        return masks, present


class ResidentBatch(api.ResidentBatch):
    """api.ResidentBatch (bpp_batch_upload / bpp_verify_resident / traces) uploaded from arrays.  form="packed": through
    bpp_batch_upload_packed (one bpp_packed_batch, no per-item structs); form="items": a bpp_verify_item array built with
    numpy pointer arithmetic.  Both end in the same resident batch (tests/test_gpu_packed.py).  form="device": the arrays are device
    tensors or (address, shape) pairs (or `proofs` is a DevicePackedInput and the other arrays are None), uploaded through
    bpp_batch_upload_packed_device without passing through the host; the same resident batch again (tests/test_gpu_device_inputs.py)."""

    def __init__(self, params, proofs, commitments, min_values, min_present, seed_nonces, label, form="packed", seed_present=None):
        self.params, self.engine, self.t = params, params.engine, int(params.extension_degree())
        self.handle = c_uint64()
        err = ctypes.create_string_buffer(256)
        if form == "device":
            t0 = time.perf_counter()
            inp = proofs if isinstance(proofs, DevicePackedInput) else DevicePackedInput(proofs, commitments, min_values, min_present,
                                                                                         seed_nonces, label, seed_present=seed_present)
            self.n, self.input = inp.n, inp
            inp.order_before(self.engine)
            t1 = time.perf_counter()
            if inp.item_states is not None:  # per-item transcripts: row i of inp.item_states serves item i
                rc = self.engine.lib.bpp_batch_upload_packed_device_transcripts(self.engine.ctx, params.handle, byref(inp.struct_without_transcript()),
                                                                                inp.item_states, byref(self.handle), err, 256)
            else:
                rc = self.engine.lib.bpp_batch_upload_packed_device(self.engine.ctx, params.handle, byref(inp.struct), byref(self.handle), err, 256)
            api._check(rc, self.engine.ctx, err)
            self.marshal_seconds, self.upload_seconds = t1 - t0, time.perf_counter() - t1
            return
        if form == "packed":
            t0 = time.perf_counter()
            inp = PackedInput(proofs, commitments, min_values, min_present, seed_nonces, label, seed_present=seed_present)
            self.n = inp.n
            t1 = time.perf_counter()
            rc = self.engine.lib.bpp_batch_upload_packed(self.engine.ctx, params.handle, byref(inp.struct), byref(self.handle), err, 256)
            api._check(rc, self.engine.ctx, err)
            self.marshal_seconds, self.upload_seconds = t1 - t0, time.perf_counter() - t1
            return
        t0 = time.perf_counter()
        proofs = np.ascontiguousarray(proofs, dtype=np.uint8)
        n, plen = proofs.shape
        commitments = np.ascontiguousarray(commitments, dtype=np.uint8)
        m = commitments.shape[1]
        commitments = _c(commitments, np.uint8, (n, m, 32))
        min_values = _c(min_values, np.uint64, (n, m))
        min_present = _c(min_present, np.uint8, (n, m))
        lbl = np.frombuffer(bytes(label), dtype=np.uint8).copy() if len(label) else np.zeros(1, dtype=np.uint8)
        items = np.zeros(n, dtype=_VERIFY_ITEM)
        items["proof"] = _rows(proofs)
        items["proof_len"] = plen
        items["commitments32"] = _rows(commitments)
        items["m"] = m
        items["min_values"] = _rows(min_values)
        items["min_present"] = _rows(min_present)
        if seed_nonces is not None:
            seed_nonces = _c(seed_nonces, np.uint8, (n, 32))
            items["seed_nonce32"] = _rows(seed_nonces)
        items["transcript_label"] = lbl.ctypes.data
        items["label_len"] = len(label)
        t1 = time.perf_counter()
        self.n = n
        rc = self.engine.lib.bpp_batch_upload(self.engine.ctx, params.handle, items.ctypes.data_as(POINTER(_lib.VerifyItem)), n,
                                              byref(self.handle), err, 256)
        api._check(rc, self.engine.ctx, err)
        self.marshal_seconds, self.upload_seconds = t1 - t0, time.perf_counter() - t1

    @classmethod
    def from_mixed(cls, params, inp):
        """the resident batch of a MixedInput (bpp_batch_upload_mixed) or a DeviceMixedInput (bpp_batch_upload_mixed_device): an ordinary
        resident batch -- verify_arrays, enqueue, the group calls and the traces work on it; refill takes a DeviceMixedInput of the
        same shape vector when the batch came from one"""
        self = cls.__new__(cls)
        self.params, self.engine, self.t = params, params.engine, int(params.extension_degree())
        self.handle = c_uint64()
        self.n, self.input = inp.n, inp
        err = ctypes.create_string_buffer(256)
        t0 = time.perf_counter()
        if isinstance(inp, DeviceMixedInput):
            inp.order_before(self.engine)
            fn = self.engine.lib.bpp_batch_upload_mixed_device
        else:
            fn = self.engine.lib.bpp_batch_upload_mixed
        t1 = time.perf_counter()
        if getattr(inp, "item_states", None) is not None:  # (a DeviceMixedInput with per-item transcripts)
            rc = self.engine.lib.bpp_batch_upload_mixed_device_transcripts(self.engine.ctx, params.handle, byref(inp.struct_without_transcript()),
                                                                           inp.item_states, byref(self.handle), err, 256)
        else:
            rc = fn(self.engine.ctx, params.handle, byref(inp.struct), byref(self.handle), err, 256)
        api._check(rc, self.engine.ctx, err)
        self.marshal_seconds, self.upload_seconds = t1 - t0, time.perf_counter() - t1
        return self

    def verify_arrays(self, action, chunk=0):
        """bpp_verify_resident with the masks as arrays (no per-item Python): (masks uint8 [n, t, 32], present uint8 [n])"""
        if not hasattr(self, "_masks"):
            self._masks = np.zeros((self.n, self.t, 32), dtype=np.uint8)
            self._present = np.zeros(self.n, dtype=np.uint8)
        err = ctypes.create_string_buffer(256)
        rc = self.engine.lib.bpp_verify_resident(self.engine.ctx, self.handle, int(action), chunk, self._masks.ctypes.data,
                                                 self._present.ctypes.data, err, 256)
        api._check(rc, self.engine.ctx, err)
        return self._masks, self._present

    def enqueue(self, bounds=None, chunk=0, actions=None, action=api.VerifyAction.VerifyOnly, verdicts=None, masks=None, present=None,
                states=None):
        """bpp_verify_enqueue: the stream-ordered counterpart of verify_groups_actions.  Enqueues on the engine's stream and returns an
        Enqueued at once; the per-group records and the recovered masks land in torch tensors on the engine's device -- `verdicts`
        int32 [G, 4] (code, tier, index, flags), `masks` uint8 [n, t, 32], `present` uint8 [n]; the ones not given are allocated
        (masks and present only when some group recovers) -- and are valid in stream order behind the call: on an engine made on
        torch's current stream, torch work enqueued afterwards may read them with no synchronisation in between.
        bounds: explicit group boundaries; None: equal chunks of `chunk` proofs (0: one group).  actions: one VerifyAction per
        group; None: `action` for every group.
        states (bpp_verify_enqueue_states): True, or a uint8 [n, 203] device tensor (or a raw device address) -- the advanced
        transcripts come back as `.states`, valid in stream order like the records: row i is item i's transcript after the proof
        where its group's record is Ok and the slot is live, 203 zero bytes everywhere else."""
        import torch
        dev = torch.device("cuda", int(self.engine.device))
        if bounds is not None:
            G = len(bounds) - 1
            arr = (ctypes.c_uint32 * (G + 1))(*bounds)
        else:
            cz = self.n if (chunk == 0 or chunk >= self.n) else int(chunk)
            G, arr = (self.n + cz - 1) // cz, None
        act = None if actions is None else (ctypes.c_int * len(actions))(*[int(a) for a in actions])
        if actions is not None and len(actions) != G:
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "one action per group expected")
        recovers = any(int(a) != 0 for a in actions) if actions is not None else int(action) != 0
        if verdicts is None:
            verdicts = torch.empty((max(G, 0), 4), dtype=torch.int32, device=dev)
        if masks is None and recovers:
            masks = torch.empty((self.n, self.t, 32), dtype=torch.uint8, device=dev)
        if present is None and recovers:
            present = torch.empty((self.n,), dtype=torch.uint8, device=dev)

        def addr(a, name, dtype, shape):
            if a is None:
                return None
            if not hasattr(a, "data_ptr"):  # (a raw address: the engine checks what lies behind it)
                return ctypes.c_void_p(int(a))
            if a.dtype != dtype or tuple(a.shape) != shape or not a.is_contiguous():
                raise api.ProofError(api.ProofErrorKind.InvalidArgument, "%s: a contiguous %s tensor of shape %s expected" % (name, dtype, shape))
            return ctypes.c_void_p(a.data_ptr())

        ticket = c_uint64()
        if states is not None and states is not False:
            if states is True:
                states = torch.empty((self.n, 203), dtype=torch.uint8, device=dev)
            rc = self.engine.lib.bpp_verify_enqueue_states(self.engine.ctx, self.handle, arr, G, int(chunk), act, int(action),
                                                           addr(verdicts, "verdicts", torch.int32, (G, 4)),
                                                           addr(masks, "masks", torch.uint8, (self.n, self.t, 32)),
                                                           addr(present, "present", torch.uint8, (self.n,)),
                                                           addr(states, "states", torch.uint8, (self.n, 203)), byref(ticket))
            api._check(rc, self.engine.ctx)
            return Enqueued(self.engine, ticket.value, G, verdicts, masks, present, states)
        rc = self.engine.lib.bpp_verify_enqueue(self.engine.ctx, self.handle, arr, G, int(chunk), act, int(action),
                                                addr(verdicts, "verdicts", torch.int32, (G, 4)),
                                                addr(masks, "masks", torch.uint8, (self.n, self.t, 32)),
                                                addr(present, "present", torch.uint8, (self.n,)), byref(ticket))
        api._check(rc, self.engine.ctx)
        return Enqueued(self.engine, ticket.value, G, verdicts, masks, present)

    def refill(self, inp, record=None, count=None, live=None, shape_vectors=True):
        """bpp_batch_refill_enqueue: new contents of the same shape for this batch (made with form="device") from the
        DevicePackedInput `inp`, enqueued on the engine's stream; an enqueue() afterwards gives what it would give on a fresh upload
        of those arrays.  Nothing is synchronised here: what wrote the arrays must be ordered before the engine's stream (an engine
        made on torch's current stream has that by construction).  The batch keeps its transcript: inp's label and state are not
        passed on.  `record`: an int32 [4] device tensor (code, message id, index, flags) or a raw address; None: allocated.  Returns a
        Refilled.  A refilled batch takes enqueued calls only.
        `count` (bpp_batch_refill_enqueue_count): the live count -- items at and beyond it are dead slots, not read, and an enqueue()
        afterwards gives, for every group with a live item, what it gives on a fresh upload of the first `count` items with the
        boundaries clipped; a group without one gets a VERDICT_EMPTY record.  An int goes into a one-word device tensor the batch
        owns (an asynchronous copy on torch's current stream: use an engine made on that stream); a device tensor of one int32 or
        uint32 word is passed as it is and read when the refill runs on the stream.  None: every item.
        `live` (bpp_batch_refill_enqueue_live; not together with `count`): a per-item live mask, a contiguous uint8 device tensor of n
        bytes (or a raw device address), read when the refill runs on the stream -- byte i non-zero: item i is live.  Dead slots
        may lie anywhere; an enqueue() afterwards gives, for every group with a live item, what it gives on a fresh upload of the
        group's live items alone, with `index` a slot offset inside the group, and a VERDICT_EMPTY record for a group without one.
        The batch keeps its own copy: the tensor may be overwritten as soon as the refill has run.  None: every item.
        A DeviceMixedInput `inp` (bpp_batch_refill_enqueue_mixed) refills a batch made by from_mixed from a DeviceMixedInput: its
        proof_lens and m must repeat the batch's vectors, its strides are the source's own; `count` and `live` mean what they mean
        above, with the fresh mixed upload of the rows in question as the reference.  shape_vectors=False passes no proof_lens / m at
        all ("the batch's own"): the steady-state form, in which the call touches nothing of size n on the host.
        An `inp` made with item_states= (bpp_batch_refill_enqueue_transcripts / _mixed_transcripts) refills a batch that was uploaded
        with per-item transcripts, and only such a batch: every refill brings the rows of its items, `count` and `live` as above."""
        import torch
        if live is None and count is None:
            live = getattr(inp, "live", None)  # (ProveEnqueued.as_mixed_input: the prover's ok mask comes with the outputs)
        if live is not None and count is not None:
            raise api.ProofError(api.ProofErrorKind.InvalidArgument, "count and live: a refill takes a live count or a live mask, not both")
        dev = torch.device("cuda", int(self.engine.device))
        live_addr = None
        if live is not None and hasattr(live, "data_ptr"):
            if live.dtype != torch.uint8 or live.numel() != self.n or not live.is_contiguous():
                raise api.ProofError(api.ProofErrorKind.InvalidArgument, "live: a contiguous uint8 tensor of n bytes expected")
            live_addr = ctypes.c_void_p(live.data_ptr())
            self._live_arg = live  # (stays alive until the refill has run)
        elif live is not None:
            live_addr = ctypes.c_void_p(int(live))
        count_addr = None
        if count is not None and hasattr(count, "data_ptr"):
            if count.dtype not in (torch.int32, torch.uint32) or count.numel() != 1:
                raise api.ProofError(api.ProofErrorKind.InvalidArgument, "count: an int or a tensor of one 32-bit word expected")
            count_addr = ctypes.c_void_p(count.data_ptr())
            self._count_arg = count  # (stays alive until the refill has run)
        elif count is not None:
            if not 0 <= int(count) < 2 ** 32:
                raise api.ProofError(api.ProofErrorKind.InvalidArgument, "count: a 32-bit unsigned value expected")
            if getattr(self, "_count_words", None) is None:
                self._count_words, self._count_next = torch.zeros((16,), dtype=torch.int32, device=dev), 0
            cur = torch.cuda.current_stream(int(self.engine.device))
            shared = bool(self.engine.stream) and int(cur.cuda_stream) == self.engine.stream
            # on the engine's own stream one word serves every refill; otherwise the write is completed here and the words take
            # turns, so that a refill still in flight keeps the word it was given
            slot = 0 if shared else self._count_next % 16
            self._count_next += 1
            word = self._count_words[slot:slot + 1]
            word.fill_(int(count) if int(count) < 2 ** 31 else int(count) - 2 ** 32)
            if not shared:
                cur.synchronize()
            count_addr = ctypes.c_void_p(word.data_ptr())
        if record is None:
            record = torch.empty((4,), dtype=torch.int32, device=dev)
        if hasattr(record, "data_ptr"):
            if record.dtype != torch.int32 or tuple(record.shape) != (4,) or not record.is_contiguous():
                raise api.ProofError(api.ProofErrorKind.InvalidArgument, "record: a contiguous int32 tensor of shape (4,) expected")
            addr = ctypes.c_void_p(record.data_ptr())
        else:
            addr = ctypes.c_void_p(int(record))
        ticket = c_uint64()
        if isinstance(inp, DeviceMixedInput):  # (first: it subclasses DevicePackedInput, whose struct goes to the packed calls below)
            st = _lib.MixedBatch.from_buffer_copy(inp.struct)
            st.transcript_state, st.transcript_label, st.label_len = None, None, 0
            if not shape_vectors:
                st.proof_lens, st.m = None, None
            if inp.item_states is not None:
                rc = self.engine.lib.bpp_batch_refill_enqueue_mixed_transcripts(self.engine.ctx, self.handle, byref(st), inp.item_states, count_addr,
                                                                                live_addr, addr, byref(ticket))
            else:
                rc = self.engine.lib.bpp_batch_refill_enqueue_mixed(self.engine.ctx, self.handle, byref(st), count_addr, live_addr, addr, byref(ticket))
            api._check(rc, self.engine.ctx)
            self.input = inp
            return Refilled(self.engine, ticket.value, record)
        st = _lib.PackedBatch.from_buffer_copy(inp.struct)
        st.transcript_state, st.transcript_label, st.label_len = None, None, 0
        if inp.item_states is not None:
            rc = self.engine.lib.bpp_batch_refill_enqueue_transcripts(self.engine.ctx, self.handle, byref(st), inp.item_states, count_addr, live_addr,
                                                                      addr, byref(ticket))
        elif live_addr is not None:
            rc = self.engine.lib.bpp_batch_refill_enqueue_live(self.engine.ctx, self.handle, byref(st), live_addr, addr, byref(ticket))
        elif count_addr is None:
            rc = self.engine.lib.bpp_batch_refill_enqueue(self.engine.ctx, self.handle, byref(st), addr, byref(ticket))
        else:
            rc = self.engine.lib.bpp_batch_refill_enqueue_count(self.engine.ctx, self.handle, byref(st), count_addr, addr, byref(ticket))
        api._check(rc, self.engine.ctx)
        self.input = inp  # (the arrays stay alive until the refill has run)
        return Refilled(self.engine, ticket.value, record)

    def enqueue_weights(self, out=None):
        """bpp_enqueue_weights, a diagnostic: the batch weights the last enqueue() of this batch used, uint8 [n, 32] on the engine's
        device, valid in stream order behind the call (dead slots of a refill with a count: zeros).  Does not wait.  Returns an
        EnqueuedWeights: `.weights` and the ticket."""
        import torch
        if out is None:
            out = torch.empty((self.n, 32), dtype=torch.uint8, device=torch.device("cuda", int(self.engine.device)))
        if hasattr(out, "data_ptr"):
            if out.dtype != torch.uint8 or tuple(out.shape) != (self.n, 32) or not out.is_contiguous():
                raise api.ProofError(api.ProofErrorKind.InvalidArgument, "out: a contiguous uint8 tensor of shape (n, 32) expected")
            addr = ctypes.c_void_p(out.data_ptr())
        else:
            addr = ctypes.c_void_p(int(out))
        ticket = c_uint64()
        api._check(self.engine.lib.bpp_enqueue_weights(self.engine.ctx, self.handle, addr, byref(ticket)), self.engine.ctx)
        return EnqueuedWeights(self.engine, ticket.value, out)


VERDICT_WRITTEN, VERDICT_REDRAW, VERDICT_REFILL, VERDICT_EMPTY = 1, 2, 4, 8
REFILL_WRITTEN, REFILL_FINDING, REFILL_FALLBACK, REFILL_COUNT = 1, 2, 4, 8


class EnqueuedWeights:
    """What ResidentBatch.enqueue_weights returns: `.weights` (uint8 [n, 32], a device tensor valid in stream order behind the call)
    and the ticket: wait() blocks until the copy has run, numpy() waits and copies the weights to the host."""

    def __init__(self, engine, ticket, weights):
        self.engine, self.ticket, self.weights = engine, ticket, weights

    def wait(self):
        api._check(self.engine.lib.bpp_enqueue_wait(self.engine.ctx, self.ticket), self.engine.ctx)

    def numpy(self):
        self.wait()
        return self.weights.cpu().numpy()


class Refilled:
    """What ResidentBatch.refill returns: `.record` (int32 [4]: code, message id, index, flags -- a device tensor, valid in stream
    order behind the call) and the ticket: done() is one event query, wait() blocks until the refill has run, result() waits,
    copies the record back and returns {"code", "tier", "index", "msg", "flags"} (bpp_refill_result: a finding has the blocking
    upload's code, index and text under tier 1; a fall-back record claims nothing and says so)."""

    def __init__(self, engine, ticket, record):
        self.engine, self.ticket, self.record = engine, ticket, record

    def done(self):
        d = ctypes.c_int()
        api._check(self.engine.lib.bpp_enqueue_done(self.engine.ctx, self.ticket, byref(d)), self.engine.ctx)
        return bool(d.value)

    def wait(self):
        api._check(self.engine.lib.bpp_enqueue_wait(self.engine.ctx, self.ticket), self.engine.ctx)

    def result(self):
        self.wait()
        host = np.ascontiguousarray(self.record.cpu().numpy())
        r = _lib.ShardResult()
        api._check(self.engine.lib.bpp_refill_result(host.ctypes.data_as(POINTER(_lib.DeviceRefill)), byref(r)), None)
        return {"code": r.code, "tier": r.tier, "index": r.index, "msg": r.msg.decode(errors="replace"), "flags": int(host[3])}


def refill_stats(engine):
    """bpp_refill_stats as a dict: calls, first_calls, host_waits"""
    s = _lib.RefillStats()
    api._check(engine.lib.bpp_refill_stats(engine.ctx, byref(s)), engine.ctx)
    return {n: int(getattr(s, n)) for n, _ in _lib.RefillStats._fields_}


class Enqueued:
    """What ResidentBatch.enqueue returns: `.verdicts` (int32 [G, 4]: code, tier, index, flags), `.masks`, `.present` -- device
    tensors, valid in stream order behind the call -- and the ticket: done() is one event query, wait() blocks until the call's
    results are there, results() waits, copies the records back and returns the dicts of verify_groups_actions (a group whose
    record carries VERDICT_REDRAW claims nothing: code 0, tier 0, and a message that says so; redraws() lists those groups)."""

    def __init__(self, engine, ticket, n_groups, verdicts, masks, present, states=None):
        self.engine, self.ticket, self.n_groups = engine, ticket, n_groups
        self.verdicts, self.masks, self.present = verdicts, masks, present
        self.states = states  # (enqueue(states=...): uint8 [n, 203], the advanced transcripts; None otherwise)

    def done(self):
        d = ctypes.c_int()
        api._check(self.engine.lib.bpp_enqueue_done(self.engine.ctx, self.ticket, byref(d)), self.engine.ctx)
        return bool(d.value)

    def wait(self):
        api._check(self.engine.lib.bpp_enqueue_wait(self.engine.ctx, self.ticket), self.engine.ctx)

    def _records(self):
        self.wait()
        host = np.ascontiguousarray(self.verdicts.cpu().numpy())
        return host.ctypes.data_as(POINTER(_lib.DeviceVerdict)), host

    def results(self):
        recs, _keep = self._records()
        out = []
        for g in range(self.n_groups):
            r = _lib.ShardResult()
            api._check(self.engine.lib.bpp_verdict_result(byref(recs[g]), byref(r)), None)
            out.append({"code": r.code, "tier": r.tier, "index": r.index, "msg": r.msg.decode(errors="replace")})
        return out

    def redraws(self):
        _recs, host = self._records()
        return [g for g in range(self.n_groups) if int(host[g, 3]) & VERDICT_REDRAW]


def enqueue_stats(engine):
    """bpp_enqueue_stats as a dict: calls, groups, host_waits, layouts_in_call"""
    s = _lib.EnqueueStats()
    api._check(engine.lib.bpp_enqueue_stats(engine.ctx, byref(s)), engine.ctx)
    return {n: int(getattr(s, n)) for n, _ in _lib.EnqueueStats._fields_}
