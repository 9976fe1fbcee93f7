"""Python mirror of the reference's ulvt_gpu / sumcheck library surface over the C-ABI.

The product is the C-ABI shared library (binius-ntt_amd/lib/libbinius_ntt_amd.so, declared in
include/binius_ntt_amd.h); this module binds it with ctypes and mirrors the reference's C++
classes so parity tests read like the reference's own:

  NTTData, DataOrder                  src/ulvt/ntt/nttconf.cuh:9-21
  AdditiveNTTConf(log_h, log_rate)    src/ulvt/ntt/nttconf.cuh:49-60
  AdditiveNTT(conf).apply(in, out)    src/ulvt/ntt/additive_ntt.cuh:175-265
  Sumcheck(num_vars, d, transposed)   src/ulvt/sumcheck/sumcheck.cuh:10-301
  check_gpu_capabilities()            src/ulvt/utils/common.cu:6-43

Device buffers are torch tensors (PyTorch-ROCm is only plumbing here: memory, streams,
torch.distributed). There is no CPU fallback: if the library is missing every call raises.
"""
import ctypes
import enum
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(os.path.dirname(_HERE))  # binius-ntt_amd/
LIB_PATH = os.environ.get("BINIUS_NTT_AMD_LIB") or os.path.join(PKG_ROOT, "lib", "libbinius_ntt_amd.so")  # env: A/B experiments
HEADER_PATH = os.path.join(os.path.dirname(PKG_ROOT), "include", "binius_ntt_amd.h")

BN_OK, BN_ERR_INVALID, BN_ERR_HIP, BN_ERR_UNSUPPORTED, BN_ERR_ALLOC = 0, 1, 2, 3, 4
_ERRNAMES = {1: "BN_ERR_INVALID", 2: "BN_ERR_HIP", 3: "BN_ERR_UNSUPPORTED", 4: "BN_ERR_ALLOC"}

_lib = None


class BnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (_ERRNAMES.get(code, code), msg))
        self.code = code


def lib():
    """Load the HIP engine. Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libbinius_ntt_amd.so not built (run `make -C binius-ntt_amd` or __graft_entry__.build())")
    # One HIP runtime per process: torch bundles its own libamdhip64 with the same SONAME as
    # ROCm's. If this library were loaded first it would pull in ROCm's copy and torch (which
    # this package uses for device buffers and streams) would then find no GPU. Import torch
    # first so that its runtime is the one both share.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, i32, u32p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)
    sig = {
        "bn_last_error": (ctypes.c_char_p, []),
        "bn_version": (ctypes.c_char_p, []),
        "bn_check_gpu_capabilities": (i32, []),
        "bn_antt_plan_create": (i32, [i32, i32, i32, i32, ctypes.POINTER(vp)]),
        "bn_antt_plan_destroy": (i32, [vp]),
        "bn_antt_forward_host": (i32, [vp, vp, sz, vp]),
        "bn_antt_forward_device": (i32, [vp, vp, vp, sz, vp]),
        "bn_antt_inverse_device": (i32, [vp, vp, vp, i32, sz, vp]),
        "bn_antt_inverse_host": (i32, [vp, vp, sz, i32, vp]),
        "bn_antt_fri_fold_device": (i32, [vp, vp, vp, i32, i32, u32p, sz, vp]),
        "bn_antt_fri_fold_host": (i32, [vp, vp, sz, i32, i32, u32p, vp]),
        "bn_antt_fri_fold_leaf": (i32, [i32, i32, i32, i32, ctypes.c_uint64, u32p, u32p, u32p]),
        "bn_antt_get_subspace_evals": (i32, [vp, u32p, sz]),
        "bn_antt_plan_query": (i32, [vp, i32, ctypes.POINTER(ctypes.c_int64)]),
        "bn_antt_plan_set_variant": (i32, [vp, i32]),
        "bn_antt_set_event_timing": (i32, [vp, i32]),
        "bn_antt_get_event_timing": (i32, [vp, ctypes.POINTER(ctypes.c_float), i32, ctypes.POINTER(i32)]),
        "bn_antt_time_passes": (i32, [vp, vp, vp, sz, i32, vp, ctypes.POINTER(ctypes.c_float), i32, ctypes.POINTER(i32)]),
        "bn_antt_pass_kernel_name": (i32, [vp, i32, ctypes.c_char_p, sz]),
        "bn_antt_inword_tables": (i32, [i32, i32, u32p, sz]),
        "bn_antt_stage_classes": (i32, [i32, i32, ctypes.POINTER(ctypes.c_int32), sz]),
        "bn_gf128_mul_device": (i32, [vp, vp, vp, sz, vp]),
        "bn_gf128_mul_bitsliced_device": (i32, [vp, vp, vp, sz, vp]),
        "bn_gf32_mul_device": (i32, [vp, vp, vp, sz, vp]),
        "bn_gf128_mul_repeat_device": (i32, [i32, vp, vp, sz, i32, vp]),
        "bn_bitslice_device": (i32, [vp, sz, i32, vp]),
        "bn_bit_reverse_device": (i32, [vp, vp, i32, sz, i32, vp]),
        "bn_bit_reverse_host": (i32, [i32, u32p, i32, i32, u32p]),
        "bn_bit_reverse_device_split": (i32, [vp, vp, i32, sz, i32, i32, vp]),
        "bn_multiply_unrolled": (i32, [i32, u32p, u32p, u32p]),
        "bn_multiply_unrolled_device": (i32, [i32, vp, vp, vp, sz, vp]),
        "bn_circuit_device": (i32, [i32, vp, vp, vp, sz, vp]),
        "bn_mul_binary_tower_32b_simd": (i32, [i32, ctypes.c_uint32, ctypes.c_uint32, u32p]),
        "bn_interleave_32b": (i32, [i32, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p]),
        "bn_xor_adjacent_32b": (i32, [i32, ctypes.c_uint32, u32p]),
        "bn_packed32_device": (i32, [i32, i32, vp, vp, vp, vp, sz, vp]),
        "bn_sumcheck_create": (i32, [i32, i32, i32, i32, u32p, ctypes.POINTER(vp)]),
        "bn_sumcheck_create_device": (i32, [i32, i32, i32, i32, vp, i32, ctypes.POINTER(vp)]),
        "bn_sumcheck_create_staged": (i32, [i32, i32, i32, i32, u32p, ctypes.POINTER(vp)]),
        "bn_sumcheck_prepare": (i32, [vp]),
        "bn_sumcheck_round_messages": (i32, [vp, u32p, u32p]),
        "bn_sumcheck_move_to_next_round": (i32, [vp, u32p]),
        "bn_sumcheck_round": (i32, [vp, ctypes.POINTER(i32)]),
        "bn_sumcheck_set_shard": (i32, [vp, i32, i32]),
        "bn_sumcheck_create_shard_device": (i32, [i32, i32, i32, i32, i32, vp, vp, ctypes.POINTER(vp)]),
        "bn_sumcheck_needs_gather": (i32, [vp, ctypes.POINTER(i32)]),
        "bn_sumcheck_set_message_sink": (i32, [vp, vp]),
        "bn_sumcheck_round_messages_sink": (i32, [vp]),
        "bn_sumcheck_stream": (i32, [vp, ctypes.POINTER(vp)]),
        "bn_sumcheck_export_shard": (i32, [vp, u32p, sz]),
        "bn_sumcheck_import_gathered": (i32, [vp, u32p, sz, i32]),
        "bn_sumcheck_destroy": (i32, [vp]),
        "bn_multilinear_composition_eval": (i32, [i32, i32, i32, i32, u32p, u32p, u32p]),
        "bn_multilinear_composition_eval_device": (i32, [i32, i32, i32, i32, vp, u32p, u32p]),
        "bn_sumcheck_interpolate": (i32, [u32p, i32, u32p, u32p]),
        "bn_eq_expand_device": (i32, [i32, u32p, u32p, vp, i32, vp]),
        "bn_eq_expand_host": (i32, [i32, i32, u32p, u32p, i32, u32p]),
        "bn_eq_eval": (i32, [i32, u32p, u32p, u32p]),
        "bn_eq_expand_device_split": (i32, [i32, u32p, u32p, vp, i32, i32, vp]),
        "bn_eq_expand_passes": (i32, [i32, i32, ctypes.POINTER(ctypes.c_int32), sz, ctypes.POINTER(i32)]),
        "bn_rs_partial_evals_device": (i32, [vp, vp, i32, vp, vp]),
        "bn_rs_partial_evals_host": (i32, [i32, u32p, u32p, i32, u32p]),
        "bn_rs_partial_evals_device_split": (i32, [vp, vp, i32, vp, sz, vp]),
        "bn_gf128_linear_map_device": (i32, [vp, vp, sz, u32p, i32, vp]),
        "bn_gf128_linear_map_host": (i32, [i32, u32p, sz, u32p, i32, u32p]),
        "bn_rs_batch_table": (i32, [u32p, u32p]),
        "bn_rs_row_check": (i32, [u32p, u32p, u32p]),
        "bn_rs_sumcheck_claim": (i32, [u32p, u32p, u32p]),
        "bn_rs_eq_eval": (i32, [i32, u32p, u32p, u32p, u32p]),
        "bn_merkle_tree_digests": (i32, [i32, ctypes.POINTER(sz)]),
        "bn_merkle_open_bytes": (i32, [i32, i32, ctypes.POINTER(sz)]),
        "bn_merkle_row_offset": (i32, [i32, i32, ctypes.POINTER(sz)]),
        "bn_merkle_commit_device": (i32, [vp, i32, i32, vp, vp]),
        "bn_merkle_commit_device_split": (i32, [vp, i32, i32, vp, i32, vp]),
        "bn_merkle_commit_host": (i32, [i32, vp, i32, i32, vp]),
        "bn_merkle_open_device": (i32, [vp, vp, i32, i32, vp, sz, vp, vp]),
        "bn_merkle_hash_leaf": (i32, [vp, i32, vp]),
        "bn_merkle_hash_node": (i32, [vp, vp, vp]),
        "bn_merkle_verify": (i32, [vp, i32, i32, ctypes.c_uint64, vp, ctypes.POINTER(i32)]),
        "bn_merkle_commit_passes": (i32, [i32, i32, i32, ctypes.POINTER(ctypes.c_int32), sz, ctypes.POINTER(i32)]),
        "bn_bb31_ntt_plan_create": (i32, [i32, ctypes.c_uint32, i32, i32, ctypes.POINTER(vp)]),
        "bn_bb31_ntt_plan_destroy": (i32, [vp]),
        "bn_bb31_ntt_forward_host": (i32, [vp, vp, sz, vp, i32]),
        "bn_bb31_ntt_forward_device": (i32, [vp, vp, vp, sz, i32, vp]),
        "bn_qm31_sumcheck_create": (i32, [i32, i32, u32p, ctypes.POINTER(vp)]),
        "bn_qm31_sumcheck_round_messages": (i32, [vp, u32p]),
        "bn_qm31_sumcheck_fold": (i32, [vp, u32p]),
        "bn_qm31_sumcheck_final_values": (i32, [vp, u32p]),
        "bn_qm31_sumcheck_destroy": (i32, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _check(rc):
    if rc != BN_OK:
        raise BnError(rc, lib().bn_last_error().decode())


def exported_symbols():
    """Names declared in include/binius_ntt_amd.h (used by the ABI test)."""
    import re
    with open(HEADER_PATH) as f:
        src = f.read()
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(bn_\w+)\s*\(", src, re.M)))


def check_gpu_capabilities():
    return bool(lib().bn_check_gpu_capabilities())


def _check_device_tensor(t, words, what):
    """Shape/device/contiguity check before handing a raw pointer to the C-ABI: a short or
    strided tensor would otherwise mean out-of-bounds device accesses."""
    if isinstance(t, int):
        return
    if not t.is_cuda:
        raise ValueError("%s must be a device tensor" % what)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    if t.element_size() * t.numel() < 4 * words:
        raise ValueError("%s holds %d bytes, need %d" % (what, t.element_size() * t.numel(), 4 * words))


def _ptr(t):
    """Device pointer of a torch tensor (or an int address)."""
    if isinstance(t, int):
        return ctypes.c_void_p(t)
    return ctypes.c_void_p(t.data_ptr())


def _stream(stream, device=None):
    """hipStream_t for a launch: `stream` (torch stream or raw handle) or, when None, torch's
    current stream of `device` (the plan's device, not whichever device is current)."""
    if stream is None:
        import torch
        dev = torch.device("cuda", device) if device is not None else None
        return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)


# ------------------------------------------------------------------ NTT data / config
class DataOrder(enum.IntEnum):
    """nttconf.cuh:9"""
    INVALID = -1
    IN_ORDER = 0
    BIT_REVERSED = 1


class NTTData:
    """Host-owned buffer (nttconf.cuh:11-21). `data` is a numpy array of `size` elements:
    uint32 for GF(2^32), shape (size, 4) uint32 limbs for GF(2^128)."""

    def __init__(self, size, order=DataOrder.INVALID, field_bits=32, data=None):
        self.order = DataOrder(order)
        self.size = int(size)
        self.field_bits = field_bits
        if data is not None:
            self.data = np.ascontiguousarray(data, dtype=np.uint32)
        elif field_bits == 32:
            self.data = np.zeros(self.size, np.uint32)
        else:
            self.data = np.zeros((self.size, field_bits // 32), np.uint32)

    def byte_len(self):
        return self.data.nbytes


class FanPaarTowerField:
    """Field policy tag (binary_tower.cuh:111-128): height 5 = GF(2^32), height 7 = GF(2^128)."""

    def __init__(self, height):
        assert height in (5, 7), "the NTT is built for GF(2^32) and GF(2^128)"
        self.height = height

    def N_BITS(self):
        return 1 << self.height


class AdditiveNTTConf:
    """nttconf.cuh:49-60; the reference ASSERTs (aborts) on bad parameters, this raises."""

    def __init__(self, log_h, log_rate, field=FanPaarTowerField(5), device=0):
        if not log_h >= 1:
            raise ValueError("log_h must be >= 1")
        if not (0 <= log_rate <= 4):
            raise ValueError("log_rate must be in [0, 4]")
        if not log_h + log_rate <= field.N_BITS():
            raise ValueError("log_h + log_rate must be <= N_BITS")
        self.log_h, self.log_rate, self.field, self.device = log_h, log_rate, field, device


class AdditiveNTT:
    """additive_ntt.cuh:175-319 over the C-ABI plan."""

    def __init__(self, conf):
        self.conf = conf
        self.field_bits = conf.field.N_BITS()
        p = ctypes.c_void_p()
        _check(lib().bn_antt_plan_create(conf.device, self.field_bits, conf.log_h, conf.log_rate, ctypes.byref(p)))
        self._plan = p

    def close(self):
        if getattr(self, "_plan", None) is not None and self._plan.value:
            lib().bn_antt_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def limbs(self):
        return self.field_bits // 32

    def apply(self, inp, out):
        """Reference semantics (additive_ntt.cuh:201-265): False (no other effect) unless
        inp.size == 2^log_h and inp.order == IN_ORDER; fills out (coset-major) synchronously."""
        n = 1 << self.conf.log_h
        if inp.size != n or inp.order != DataOrder.IN_ORDER:
            return False
        src = np.ascontiguousarray(inp.data, dtype=np.uint32)
        assert src.size == n * self.limbs
        n_out = n << self.conf.log_rate
        if out.data.size != n_out * self.limbs:
            out.data = np.zeros((n_out,) if self.limbs == 1 else (n_out, self.limbs), np.uint32)
            out.size = n_out
        dst = out.data
        _check(lib().bn_antt_forward_host(self._plan, src.ctypes.data, n, dst.ctypes.data))
        out.order = DataOrder.IN_ORDER
        return True

    def forward_device(self, d_in, d_out, batch=1, stream=None):
        """Device-resident transform(s) on torch tensors (or raw addresses); async on `stream`
        (default: torch's current stream of the plan's device)."""
        n = (1 << self.conf.log_h) * self.limbs * batch
        _check_device_tensor(d_in, n, "d_in")
        _check_device_tensor(d_out, n << self.conf.log_rate, "d_out")
        _check(lib().bn_antt_forward_device(self._plan, _ptr(d_in), _ptr(d_out), batch,
                                            _stream(stream, self.conf.device)))

    def inverse(self, inp, out, coset=0):
        """Evaluations on coset `coset` (block `coset` of apply()'s output) back to coefficients;
        no reference counterpart. False (no other effect) unless inp.size == 2^log_h and
        inp.order == IN_ORDER; fills out with 2^log_h elements synchronously."""
        n = 1 << self.conf.log_h
        if inp.size != n or inp.order != DataOrder.IN_ORDER:
            return False
        src = np.ascontiguousarray(inp.data, dtype=np.uint32)
        assert src.size == n * self.limbs
        dst = out.data
        if dst.size != n * self.limbs:
            dst = np.zeros((n,) if self.limbs == 1 else (n, self.limbs), np.uint32)
        _check(lib().bn_antt_inverse_host(self._plan, src.ctypes.data, n, coset, dst.ctypes.data))
        out.data = dst
        out.size = n
        out.order = DataOrder.IN_ORDER
        return True

    def inverse_device(self, d_in, d_out, coset=0, batch=1, stream=None):
        """Device-resident inverse transform(s), every one on coset `coset`; async on `stream`
        (default: torch's current stream of the plan's device). d_in is left untouched."""
        n = (1 << self.conf.log_h) * self.limbs * batch
        _check_device_tensor(d_in, n, "d_in")
        _check_device_tensor(d_out, n, "d_out")
        _check(lib().bn_antt_inverse_device(self._plan, _ptr(d_in), _ptr(d_out), coset, batch,
                                            _stream(stream, self.conf.device)))

    @staticmethod
    def _challenges(challenges):
        ch = np.ascontiguousarray(challenges, dtype=np.uint32)
        if ch.ndim != 2 or ch.shape[1] != 4:
            raise ValueError("challenges must be an (arity, 4) uint32 array")
        return ch, ch.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))

    def fri_fold(self, inp, out, round, challenges):
        """FRI-Binius fold of one host codeword at round `round` (bn_antt_fri_fold_host) with the
        (arity, 4) uint32 `challenges`, challenges[0] first; no reference counterpart. False (no
        other effect) unless inp.size == 2^(log_h+log_rate-round) and inp.order == IN_ORDER; fills
        out with inp.size >> arity elements synchronously."""
        ch, chp = self._challenges(challenges)
        log_in = self.conf.log_h + self.conf.log_rate - round
        if round < 0 or log_in < 0 or inp.size != 1 << log_in or inp.order != DataOrder.IN_ORDER:
            return False
        src = np.ascontiguousarray(inp.data, dtype=np.uint32)
        assert src.size == inp.size * self.limbs
        n_out = inp.size >> len(ch)
        dst = out.data
        if dst.size != n_out * self.limbs:
            dst = np.zeros((n_out,) if self.limbs == 1 else (n_out, self.limbs), np.uint32)
        _check(lib().bn_antt_fri_fold_host(self._plan, src.ctypes.data, inp.size, round, len(ch), chp, dst.ctypes.data))
        out.data = dst
        out.size = n_out
        out.order = DataOrder.IN_ORDER
        return True

    def fri_fold_device(self, d_in, d_out, round, challenges, batch=1, stream=None):
        """Device-resident fold of `batch` codewords of round `round` with the (arity, 4) uint32
        host array `challenges` (the arity is its length), in one launch; async on `stream`
        (default: torch's current stream of the plan's device). d_in is left untouched."""
        ch, chp = self._challenges(challenges)
        if round >= 0 and len(ch) >= 1 and round + len(ch) <= self.conf.log_h:  # else: the library's own error
            n = (1 << (self.conf.log_h + self.conf.log_rate - round)) * self.limbs * batch
            _check_device_tensor(d_in, n, "d_in")
            _check_device_tensor(d_out, n >> len(ch), "d_out")
        _check(lib().bn_antt_fri_fold_device(self._plan, _ptr(d_in), _ptr(d_out), round, len(ch), chp, batch,
                                             _stream(stream, self.conf.device)))

    def subspace_evals(self):
        lh, w = self.conf.log_h, self.conf.log_h + self.conf.log_rate - 1
        out = np.zeros(max(1, lh * w), np.uint32)
        _check(lib().bn_antt_get_subspace_evals(self._plan, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), out.size))
        return out[: lh * w].reshape(lh, w)

    def variant(self):
        v = ctypes.c_int64()
        _check(lib().bn_antt_plan_query(self._plan, 4, ctypes.byref(v)))
        return v.value

    def set_variant(self, variant):
        """0: compact tiles, per-butterfly twiddles (default for log_h < 12); 1: bitsliced LDS tiles;
        4: bitsliced register tiles (three to four waves per SIMD) on every pass; 5: register tiles
        for the GF(2^8)-twiddle passes, LDS tiles for the others (default for log_h >= 12).
        Variants 1, 4 and 5 need log_h >= 12; results are identical."""
        _check(lib().bn_antt_plan_set_variant(self._plan, variant))

    def set_event_timing(self, enable):
        _check(lib().bn_antt_set_event_timing(self._plan, 1 if enable else 0))

    def pass_kernel_name(self, i):
        """Demangled name of the kernel pass i launches (bn_antt_pass_kernel_name)."""
        buf = ctypes.create_string_buffer(512)
        _check(lib().bn_antt_pass_kernel_name(self._plan, i, buf, 512))
        return buf.value.decode()

    def time_passes(self, d_in, d_out, reps=10, batch=1, stream=None):
        """Steady-state ms per launch of each pass (bn_antt_time_passes); d_out is scratch."""
        n = (1 << self.conf.log_h) * self.limbs * batch
        _check_device_tensor(d_in, n, "d_in")
        _check_device_tensor(d_out, n << self.conf.log_rate, "d_out")
        arr = (ctypes.c_float * 16)()
        k = ctypes.c_int()
        _check(lib().bn_antt_time_passes(self._plan, _ptr(d_in), _ptr(d_out), batch, reps,
                                         _stream(stream, self.conf.device), arr, 16, ctypes.byref(k)))
        return [arr[i] for i in range(min(k.value, 16))]

    def event_timing(self):
        arr = (ctypes.c_float * 16)()
        n = ctypes.c_int()
        _check(lib().bn_antt_get_event_timing(self._plan, arr, 16, ctypes.byref(n)))
        return [arr[i] for i in range(min(n.value, 16))]


# ------------------------------------------------------------------ BabyBear NTT (prime-field sibling)
class BB31:
    """risc0::Fp value (src/ulvt/finite_fields/risc0_baby_bear.h:40-190), canonical int view:
    BB31(r) == r mod p, asUInt32() returns the canonical value."""
    P = 15 * (1 << 27) + 1

    def __init__(self, v=0):
        self.v = int(v) % self.P

    def asUInt32(self):
        return self.v

    def __mul__(self, o):
        return BB31(self.v * o.v)

    def __add__(self, o):
        return BB31(self.v + o.v)

    def __sub__(self, o):
        return BB31(self.v - o.v)

    def __eq__(self, o):
        return isinstance(o, BB31) and self.v == o.v

    @staticmethod
    def pow(x, n):
        return BB31(pow(x.v, int(n), BB31.P))

    @staticmethod
    def inv(x):
        return BB31(pow(x.v, BB31.P - 2, BB31.P))

    @staticmethod
    def one():
        return BB31(1)


class NTTConfRad2:
    """nttconf.cuh:25-47; the reference ASSERTs on bad parameters, this raises."""

    def __init__(self, generator, log_group_order, log_inp_size, device=0):
        if not 1 <= log_inp_size <= 27:
            raise ValueError("log_inp_size must be in [1, 27]")
        if not log_group_order >= log_inp_size:
            raise ValueError("log_group_order must be >= log_inp_size")
        self.generator = generator if isinstance(generator, BB31) else BB31(generator)
        self.log_group_order, self.log_inp_size, self.device = log_group_order, log_inp_size, device


class NTT:
    """NTT<BB31> (gpuntt.cuh:126-209) over the C-ABI plan: natural-order DFT with
    w = generator^(2^(log_group_order - log_inp_size))."""

    def __init__(self, conf):
        self.conf = conf
        p = ctypes.c_void_p()
        _check(lib().bn_bb31_ntt_plan_create(conf.device, conf.generator.v, conf.log_group_order,
                                             conf.log_inp_size, ctypes.byref(p)))
        self._plan = p

    def close(self):
        if getattr(self, "_plan", None) is not None and self._plan.value:
            lib().bn_bb31_ntt_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, inp, out):
        """Reference semantics: input of 2^log_inp_size canonical words, IN_ORDER or
        BIT_REVERSED; output in order (raises where the reference ASSERTs)."""
        n = 1 << self.conf.log_inp_size
        if inp.size != n:
            raise ValueError("input has %d elements, plan expects %d" % (inp.size, n))
        src = np.ascontiguousarray(inp.data, dtype=np.uint32)
        if out.data.size != n:
            out.data = np.zeros(n, np.uint32)
            out.size = n
        br = 1 if inp.order == DataOrder.BIT_REVERSED else 0
        _check(lib().bn_bb31_ntt_forward_host(self._plan, src.ctypes.data, n, out.data.ctypes.data, br))
        out.order = DataOrder.IN_ORDER

    def forward_device(self, d_in, d_out, batch=1, bit_reversed=False, stream=None):
        _check(lib().bn_bb31_ntt_forward_device(self._plan, _ptr(d_in), _ptr(d_out), batch,
                                                1 if bit_reversed else 0, _stream(stream, self.conf.device)))


# ------------------------------------------------------------------ field / bitslicing
def _dev_index(t):
    return None if isinstance(t, int) else t.device.index


def _same_size(what, *ts):
    sizes = {t.numel() * t.element_size() for t in ts if not isinstance(t, int)}
    if len(sizes) > 1:
        raise ValueError("%s operands differ in size: %s" % (what, sorted(sizes)))


def gf128_mul(a, b, out, stream=None):
    _same_size("gf128_mul", a, b, out)
    for t, w in ((a, "a"), (b, "b"), (out, "out")):
        _check_device_tensor(t, a.numel(), w)
    _check(lib().bn_gf128_mul_device(_ptr(a), _ptr(b), _ptr(out), a.numel() // 4, _stream(stream, _dev_index(a))))


def gf32_mul(a, b, out, stream=None):
    _same_size("gf32_mul", a, b, out)
    for t, w in ((a, "a"), (b, "b"), (out, "out")):
        _check_device_tensor(t, a.numel(), w)
    _check(lib().bn_gf32_mul_device(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream(stream, _dev_index(a))))


def gf128_mul_bitsliced(a, b, out, stream=None):
    _same_size("gf128_mul_bitsliced", a, b, out)
    for t, w in ((a, "a"), (b, "b"), (out, "out")):
        _check_device_tensor(t, a.numel(), w)
    _check(lib().bn_gf128_mul_bitsliced_device(_ptr(a), _ptr(b), _ptr(out), a.numel() // 128,
                                               _stream(stream, _dev_index(a))))


def gf128_mul_repeat(kind, state, operand, threads, iters, stream=None):
    _check(lib().bn_gf128_mul_repeat_device(kind, _ptr(state), _ptr(operand), threads, iters,
                                            _stream(stream, _dev_index(state))))


def bitslice(buf, untranspose=False, stream=None):
    _check_device_tensor(buf, buf.numel(), "buf")
    _check(lib().bn_bitslice_device(_ptr(buf), buf.numel() // 128, 1 if untranspose else 0,
                                    _stream(stream, _dev_index(buf))))


def bit_reverse(inp, out, log_n, batch=1, bitsliced=False, stream=None, tile_log=0):
    """bn_bit_reverse_device: out[b*2^n + rev_n(x)] = inp[b*2^n + x] for `batch` columns of 2^log_n
    compact GF(2^128) elements in device tensors (4 * batch * 2^log_n words each); bitsliced: the
    result in the layout of bitslice(), a data_is_transposed sumcheck column. `inp` is not written and
    must not overlap `out`. Async on `stream` (default: torch's current stream of inp's device).
    tile_log != 0 forces the tile's run length (bn_bit_reverse_device_split, a test hook)."""
    if 0 <= log_n <= 30 and 0 < batch <= (1 << 32) >> log_n:  # else: the library's own error
        _check_device_tensor(inp, (4 * batch) << log_n, "inp")
        _check_device_tensor(out, (4 * batch) << log_n, "out")
    st = _stream(stream, _dev_index(inp))
    if tile_log:
        _check(lib().bn_bit_reverse_device_split(_ptr(inp), _ptr(out), log_n, batch, 1 if bitsliced else 0, tile_log, st))
    else:
        _check(lib().bn_bit_reverse_device(_ptr(inp), _ptr(out), log_n, batch, 1 if bitsliced else 0, st))


def bit_reverse_host(inp, bitsliced=False, device=0):
    """bn_bit_reverse_host: the permutation of a (2^n, 4) uint32 host array as a new array of that
    shape (bitsliced: the blocks' words in that shape), synchronous. n is taken from the size."""
    a = np.ascontiguousarray(inp, dtype=np.uint32).reshape(-1, 4)
    n = a.shape[0]
    if n == 0 or n & (n - 1):
        raise ValueError("inp must hold a power of two of elements")
    out = np.zeros_like(a)
    _check(lib().bn_bit_reverse_host(device, _u32p(a), n.bit_length() - 1, 1 if bitsliced else 0, _u32p(out)))
    return out


def fri_fold_leaf(log_h, log_rate, round, index, leaf, challenges):
    """bn_antt_fri_fold_leaf: element `index` of the fold of rounds round .. round+arity-1 of a
    (log_h, log_rate) GF(2^128) codeword, from the 2^arity elements of its leaf ((2^arity, 4) uint32,
    or the leaf's bytes) and the (arity, 4) uint32 `challenges`. Host arithmetic: no plan, no device."""
    ch = np.ascontiguousarray(challenges, dtype=np.uint32)
    if ch.ndim != 2 or ch.shape[1] != 4:
        raise ValueError("challenges must be an (arity, 4) uint32 array")
    lf = np.frombuffer(bytes(leaf), dtype=np.uint32) if isinstance(leaf, (bytes, bytearray)) else np.ascontiguousarray(leaf, dtype=np.uint32).reshape(-1)
    if 1 <= len(ch) <= 8 and lf.size != 4 << len(ch):
        raise ValueError("the leaf holds %d words, need %d" % (lf.size, 4 << len(ch)))
    lf = np.ascontiguousarray(lf)
    out = np.zeros(4, np.uint32)
    if index < 0:
        raise ValueError("index must be >= 0")
    _check(lib().bn_antt_fri_fold_leaf(log_h, log_rate, round, len(ch), index, _u32p(lf), _u32p(ch) if len(ch) else None,
                                       _u32p(out)))
    return out


def multiply_unrolled(height, a, b, dst=None):
    """multiply_unrolled<HEIGHT> (binary_tower_unrolled.cuh:4-5) on host arrays of 2^height
    words (32 bitsliced products); dst may be a (alias-safe). Returns dst."""
    w = 1 << height
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    if a.size != w or b.size != w:
        raise ValueError("operands must hold 2^height = %d words" % w)
    if dst is None:
        dst = np.zeros(w, np.uint32)
    _check(lib().bn_multiply_unrolled(height, _u32p(a), _u32p(b), _u32p(dst)))
    return dst


def multiply_unrolled_device(height, a, b, out, stream=None):
    """Device batch of multiply_unrolled<height> over consecutive 2^height-word blocks."""
    _same_size("multiply_unrolled_device", a, b, out)
    w = 1 << height
    for t, nm in ((a, "a"), (b, "b"), (out, "out")):
        _check_device_tensor(t, a.numel(), nm)
    _check(lib().bn_multiply_unrolled_device(height, _ptr(a), _ptr(b), _ptr(out), a.numel() // w,
                                             _stream(stream, _dev_index(a))))


# bn_circuit_device's circuits, in the order of csrc/bitsliced_gen.hpp: (name, words of a and out
# per block, words of b, blocks that share those words of b: 64 for a wave-uniform twiddle)
CIRCUITS = (("bsm2_mul", 4, 4, 1), ("bsm3_mul", 8, 8, 1), ("bsm3x4_fma_tw", 32, 1, 1), ("bsm3x4_mul_acc", 32, 8, 1),
            ("bsm4_mul", 16, 16, 1), ("bsm4x2_fma_tw", 32, 1, 1), ("bsm4x2_mul_acc", 32, 16, 1), ("bsm5_mul", 32, 32, 1),
            ("bsm5_fma_tw", 32, 1, 1), ("bsm5_mul_acc", 32, 32, 1), ("bsm6_mul", 64, 64, 1), ("bsm7_mul", 128, 128, 1),
            ("bsm5_mul_w", 32, 1, 64), ("bsm6_fma_w2", 64, 2, 64))


def circuit_device(circuit, a, b, out, n_blocks, stream=None):
    """Test hook: generated circuit `circuit` (index into CIRCUITS) on n_blocks 32-product blocks,
    one block per lane (bn_circuit_device). out is read first by the accumulate forms."""
    if 0 <= circuit < len(CIRCUITS):
        _, wa, wb, share = CIRCUITS[circuit]
        words_b = wb * ((n_blocks + share - 1) // share)
        for t, words, nm in ((a, wa * n_blocks, "a"), (b, words_b, "b"), (out, wa * n_blocks, "out")):
            _check_device_tensor(t, words, nm)
    _check(lib().bn_circuit_device(circuit, _ptr(a), _ptr(b), _ptr(out), n_blocks, _stream(stream, _dev_index(a))))


def mul_binary_tower_32b_simd(height, a, b):
    """mul_binary_tower_32b_simd<HEIGHT>(a, b) (binary_tower_simd.cuh:77-127)."""
    out = ctypes.c_uint32()
    _check(lib().bn_mul_binary_tower_32b_simd(height, a, b, ctypes.byref(out)))
    return out.value


def interleave_32b(height, a, b):
    """interleave_32b<HEIGHT>(a, b) -> (c, d) (binary_tower_simd.cuh:129-139)."""
    c, d = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().bn_interleave_32b(height, a, b, ctypes.byref(c), ctypes.byref(d)))
    return c.value, d.value


def xor_adjacent_32b(height, a):
    """xor_adjacent_32b<HEIGHT>(a) (binary_tower_simd.cuh:141-150)."""
    out = ctypes.c_uint32()
    _check(lib().bn_xor_adjacent_32b(height, a, ctypes.byref(out)))
    return out.value


def packed32_device(op, height, a, b=None, c=None, d=None, stream=None):
    """Device batch of the packed-word primitives: op 0 multiply, 1 interleave, 2 xor_adjacent."""
    n = a.numel()
    for t, nm in ((a, "a"), (b, "b"), (c, "c"), (d, "d")):
        if t is not None:
            _check_device_tensor(t, n, nm)
    _check(lib().bn_packed32_device(op, height, _ptr(a), _ptr(b) if b is not None else None,
                                    _ptr(c), _ptr(d) if d is not None else None, n, _stream(stream, _dev_index(a))))


# ------------------------------------------------------------------ sumcheck
class Sumcheck:
    """Sumcheck<NUM_VARS, COMPOSITION_SIZE, DATA_IS_TRANSPOSED> (sumcheck.cuh:10-301)."""

    def __init__(self, num_vars, composition_size, data_is_transposed, evals, device=0, shard=None, staged=False):
        """staged=True (host evals only): copy the columns but leave compact input untransposed until
        prepare() (or the first round) — the reference constructor's separate Memcpy and Transpose
        phases (sumcheck.cuh:88-124)."""
        self.num_vars, self.d, self.device = num_vars, composition_size, device
        p = ctypes.c_void_p()
        if isinstance(evals, np.ndarray):
            ev = np.ascontiguousarray(evals, dtype=np.uint32).reshape(-1)
            create = lib().bn_sumcheck_create_staged if staged else lib().bn_sumcheck_create
            _check(create(device, num_vars, composition_size, 1 if data_is_transposed else 0,
                          ev.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(p)))
        else:
            _check_device_tensor(evals, composition_size * 4 << num_vars, "evals")
            # the library copies on its own stream: the producer (an NTT, a torch kernel) must be done.
            # A raw device address (int) carries no stream: the caller must have synchronised it.
            if not isinstance(evals, int):
                import torch
                torch.cuda.current_stream(evals.device).synchronize()
            _check(lib().bn_sumcheck_create_device(device, num_vars, composition_size,
                                                   1 if data_is_transposed else 0, _ptr(evals), 0, ctypes.byref(p)))
        self._sc = p
        self._bind()
        if shard is not None:
            _check(lib().bn_sumcheck_set_shard(self._sc, shard[0], shard[1]))

    def prepare(self):
        """The device bit-transpose of a staged prover's compact columns (synchronous; no-op otherwise)."""
        _check(lib().bn_sumcheck_prepare(self._sc))

    def _bind(self):
        # per-round calls are on the protocol's critical path (the GPU waits for the host's
        # challenge): resolve the entry points and the output buffers' pointers once
        L, u32p = lib(), ctypes.POINTER(ctypes.c_uint32)
        self._f_msgs, self._f_next = L.bn_sumcheck_round_messages, L.bn_sumcheck_move_to_next_round
        self._sum_buf = np.zeros(4, np.uint32)
        self._pts_buf = np.zeros(4 * (self.d + 1), np.uint32)
        self._ch_buf = np.zeros(4, np.uint32)
        self._sum_p, self._pts_p, self._ch_p = (b.ctypes.data_as(u32p) for b in (self._sum_buf, self._pts_buf, self._ch_buf))

    @classmethod
    def from_shard(cls, num_vars, composition_size, local_evals, rank, world, device=None, stream=None):
        """Shard prover from this rank's share only (bn_sumcheck_create_shard_device): local_evals
        is a device tensor of composition_size * 4 * 2^num_vars / world words (bitsliced batches
        b with b mod world == rank, in order); the copy is ordered after `stream`. The prover runs
        on local_evals' device (`device`, if given, must name the same one)."""
        _check_device_tensor(local_evals, composition_size * (4 << num_vars) // world, "local_evals")
        if not isinstance(local_evals, int):
            if device is None:
                device = local_evals.device.index
            elif device != local_evals.device.index:
                raise ValueError("device %d does not hold local_evals (cuda:%d)" % (device, local_evals.device.index))
        elif device is None:
            device = 0
        self = cls.__new__(cls)
        self.num_vars, self.d, self.device = num_vars, composition_size, device
        p = ctypes.c_void_p()
        _check(lib().bn_sumcheck_create_shard_device(device, num_vars, composition_size, rank, world,
                                                     _ptr(local_evals), _stream(stream, local_evals.device.index),
                                                     ctypes.byref(p)))
        self._sc = p
        self._bind()
        return self

    def this_round_messages(self):
        rc = self._f_msgs(self._sc, self._sum_p, self._pts_p)
        if rc != BN_OK:
            _check(rc)
        return self._sum_buf.copy(), self._pts_buf.reshape(self.d + 1, 4).copy()

    def move_to_next_round(self, challenge):
        self._ch_buf[:] = np.asarray(challenge, dtype=np.uint32).reshape(4)
        rc = self._f_next(self._sc, self._ch_p)
        if rc != BN_OK:
            _check(rc)

    def round(self):
        r = ctypes.c_int()
        _check(lib().bn_sumcheck_round(self._sc, ctypes.byref(r)))
        return r.value

    # sharded endgame (see bn_sumcheck_needs_gather); driven by binius_ntt_amd.distributed
    def set_message_sink(self, words):
        """bn_sumcheck_set_message_sink: later messages kernels also write the raw point words (and
        the p(1)-skipped flag at word 36) into `words`, a device tensor of >= 37 int32 (None: stop)."""
        if words is None:
            _check(lib().bn_sumcheck_set_message_sink(self._sc, None))
            self._sink = None
            return
        _check_device_tensor(words, 4 * (8 + 1) + 1, "message sink")
        self._sink = words  # keep the buffer alive while the prover writes it
        _check(lib().bn_sumcheck_set_message_sink(self._sc, _ptr(words)))

    def round_messages_sink(self):
        """bn_sumcheck_round_messages_sink: the round's messages kernel is queued (no wait); its raw
        points land in the sink on stream_handle()'s stream."""
        _check(lib().bn_sumcheck_round_messages_sink(self._sc))

    def stream_handle(self):
        """The prover's hipStream_t (as an int), for torch.cuda.ExternalStream."""
        s = ctypes.c_void_p()
        _check(lib().bn_sumcheck_stream(self._sc, ctypes.byref(s)))
        return s.value or 0

    def needs_gather(self):
        f = ctypes.c_int()
        _check(lib().bn_sumcheck_needs_gather(self._sc, ctypes.byref(f)))
        return bool(f.value)

    def export_shard(self):
        out = np.zeros(128 * self.d, np.uint32)
        _check(lib().bn_sumcheck_export_shard(self._sc, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), out.size))
        return out

    def import_gathered(self, words, world):
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        _check(lib().bn_sumcheck_import_gathered(self._sc, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), w.size,
                                                 world))

    def close(self):
        if getattr(self, "_sc", None) is not None and self._sc.value:
            lib().bn_sumcheck_destroy(self._sc)
            self._sc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _u32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def evaluate_multilinear_composition(evals, num_vars, composition_size, data_is_transposed, challenges, device=0):
    """evaluate_multilinear_composition (src/ulvt/sumcheck/test/verifier.cu:88-107) on the GPU:
    prod_j f_j(r) for the columns in `evals` (numpy host array or torch device tensor)."""
    ch = np.ascontiguousarray(challenges, dtype=np.uint32).reshape(-1)
    out = np.zeros(4, np.uint32)
    if isinstance(evals, np.ndarray):
        ev = np.ascontiguousarray(evals, dtype=np.uint32).reshape(-1)
        _check(lib().bn_multilinear_composition_eval(device, num_vars, composition_size, 1 if data_is_transposed else 0,
                                                     _u32p(ev), _u32p(ch), _u32p(out)))
    else:
        _check(lib().bn_multilinear_composition_eval_device(device, num_vars, composition_size,
                                                            1 if data_is_transposed else 0, _ptr(evals), _u32p(ch),
                                                            _u32p(out)))
    return out


def evaluate_univariate_given_points(challenge, points):
    """evaluate_univariate_given_points (verifier.cu:9-31): Lagrange interpolation through
    (k, points[k]) evaluated at `challenge` (4-word GF(2^128) values)."""
    p = np.ascontiguousarray(points, dtype=np.uint32).reshape(-1)
    c = np.ascontiguousarray(challenge, dtype=np.uint32).reshape(4)
    out = np.zeros(4, np.uint32)
    _check(lib().bn_sumcheck_interpolate(_u32p(p), p.size // 4, _u32p(c), _u32p(out)))
    return out


# ------------------------------------------------------------------ eq-indicator expansion
def _eq_args(num_vars, challenges, scale):
    """The (num_vars, 4) challenges and the 4-word scale (or None) as arrays and C pointers."""
    ch = np.ascontiguousarray(challenges, dtype=np.uint32)
    if ch.size == 0:
        ch = ch.reshape(0, 4)
    if ch.shape != (num_vars, 4):
        raise ValueError("challenges must be a (num_vars, 4) uint32 array")
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.uint32).reshape(4)
    return ch, sc, (_u32p(ch) if num_vars > 0 else None), (None if sc is None else _u32p(sc))


def eq_expand(num_vars, challenges, out, scale=None, bitsliced=False, stream=None, max_levels=0):
    """bn_eq_expand_device: E[x] = scale * prod_i (bit_{n-1-i}(x) ? r_i : 1 ^ r_i) into the device
    tensor `out` (4 * 2^num_vars words), compact or bitsliced; `challenges` is a (num_vars, 4) uint32
    host array, highest variable first. Async on `stream` (default: torch's current stream of out's
    device). max_levels != 0 forces the per-pass level cap (bn_eq_expand_device_split, a test hook)."""
    ch, sc, chp, scp = _eq_args(num_vars, challenges, scale)
    if 0 <= num_vars <= 30:  # else: the library's own error
        _check_device_tensor(out, 4 << num_vars, "out")
    st = _stream(stream, _dev_index(out))
    if max_levels:
        _check(lib().bn_eq_expand_device_split(num_vars, chp, scp, _ptr(out), 1 if bitsliced else 0, max_levels, st))
    else:
        _check(lib().bn_eq_expand_device(num_vars, chp, scp, _ptr(out), 1 if bitsliced else 0, st))


def eq_expand_host(num_vars, challenges, scale=None, bitsliced=False, device=0):
    """bn_eq_expand_host: the same into a new (2^num_vars, 4) uint32 host array (bitsliced: the
    blocks' words in that shape), synchronous."""
    ch, sc, chp, scp = _eq_args(num_vars, challenges, scale)
    out = np.zeros((1 << num_vars if 0 <= num_vars <= 30 else 1, 4), np.uint32)
    _check(lib().bn_eq_expand_host(device, num_vars, chp, scp, 1 if bitsliced else 0, _u32p(out)))
    return out


def eq_eval(a, b):
    """bn_eq_eval: prod_i (a_i b_i ^ (1 ^ a_i)(1 ^ b_i)) for two (n, 4) uint32 points (host arithmetic)."""
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 4)
    b = np.ascontiguousarray(b, dtype=np.uint32).reshape(-1, 4)
    if a.shape != b.shape:
        raise ValueError("the points differ in length")
    out = np.zeros(4, np.uint32)
    _check(lib().bn_eq_eval(a.shape[0], _u32p(a), _u32p(b), _u32p(out)))
    return out


def eq_expand_passes(num_vars, max_levels=0):
    """bn_eq_expand_passes: the levels of each pass of the expansion, first pass first (host only)."""
    levels = (ctypes.c_int32 * 32)()
    n = ctypes.c_int()
    _check(lib().bn_eq_expand_passes(num_vars, max_levels, levels, 32, ctypes.byref(n)))
    return [levels[i] for i in range(n.value)]


# ------------------------------------------------------------------ ring-switching (GF(2) witnesses)
def _rs_words(a, rows, what):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.size != 4 * rows:
        raise ValueError("%s must hold %d x 4 uint32 words (got %d words)" % (what, rows, a.size))
    return a.reshape(rows, 4)


def rs_partial_evals(packed, eq, log_n, out, stream=None, max_blocks_per_group=0):
    """bn_rs_partial_evals_device: s^_v = XOR over w with bit_v(packed[w]) = 1 of eq[w], v = 0 .. 127, for
    two bitsliced columns of 2^log_n elements in device tensors (4 * 2^log_n words each, the same element
    order) into the device tensor `out` (512 words: 128 compact elements; need not be initialised). Async
    on `stream` (default: torch's current stream of packed's device). max_blocks_per_group != 0 caps a
    work-group's run of blocks (bn_rs_partial_evals_device_split, a test hook)."""
    if 5 <= log_n <= 30:  # else: the library's own error
        _check_device_tensor(packed, 4 << log_n, "packed")
        _check_device_tensor(eq, 4 << log_n, "eq")
    _check_device_tensor(out, 512, "out")
    st = _stream(stream, _dev_index(packed))
    if max_blocks_per_group:
        _check(lib().bn_rs_partial_evals_device_split(_ptr(packed), _ptr(eq), log_n, _ptr(out), max_blocks_per_group, st))
    else:
        _check(lib().bn_rs_partial_evals_device(_ptr(packed), _ptr(eq), log_n, _ptr(out), st))


def rs_partial_evals_host(packed, eq, device=0):
    """bn_rs_partial_evals_host: the same on two (2^n, 4) uint32 host arrays holding bitsliced blocks,
    as a new (128, 4) array, synchronous. n is taken from the size."""
    a = np.ascontiguousarray(packed, dtype=np.uint32).reshape(-1, 4)
    b = np.ascontiguousarray(eq, dtype=np.uint32).reshape(-1, 4)
    n = a.shape[0]
    if n == 0 or n & (n - 1) or b.shape != a.shape:
        raise ValueError("the columns must hold the same power of two of elements")
    out = np.zeros((128, 4), np.uint32)
    _check(lib().bn_rs_partial_evals_host(device, _u32p(a), _u32p(b), n.bit_length() - 1, _u32p(out)))
    return out


def gf128_linear_map(inp, out, matrix, bitsliced=False, stream=None):
    """bn_gf128_linear_map_device: out[w] = XOR over u with bit_u(inp[w]) = 1 of matrix[u] over the whole
    device tensor `inp` (compact 4-word elements, or bitsliced 128-word blocks); `matrix` is a (128, 4)
    uint32 host array. `out` may be `inp`. Async on `stream` (default: torch's current stream of inp's
    device)."""
    m = _rs_words(matrix, 128, "matrix")
    _same_size("gf128_linear_map", inp, out)
    words = inp.numel() * inp.element_size() // 4
    unit = 128 if bitsliced else 4
    if words % unit:
        raise ValueError("inp must hold whole %s" % ("128-word blocks" if bitsliced else "elements"))
    _check_device_tensor(inp, words, "inp")
    _check_device_tensor(out, words, "out")
    _check(lib().bn_gf128_linear_map_device(_ptr(inp), _ptr(out), words // unit, _u32p(m), 1 if bitsliced else 0,
                                            _stream(stream, _dev_index(inp))))


def gf128_linear_map_host(inp, matrix, bitsliced=False, device=0):
    """bn_gf128_linear_map_host: the same on an (n, 4) uint32 host array as a new array, synchronous."""
    a = np.ascontiguousarray(inp, dtype=np.uint32).reshape(-1, 4)
    m = _rs_words(matrix, 128, "matrix")
    if bitsliced and a.shape[0] % 32:
        raise ValueError("bitsliced input must hold whole 32-element blocks")
    out = np.zeros_like(a)
    _check(lib().bn_gf128_linear_map_host(device, _u32p(a), a.shape[0] // 32 if bitsliced else a.shape[0], _u32p(m),
                                          1 if bitsliced else 0, _u32p(out)))
    return out


def rs_batch_table(r2):
    """bn_rs_batch_table: B[u] = eq(r'', u) as a (128, 4) uint32 array; r2 is (7, 4). Host arithmetic."""
    r2 = _rs_words(r2, 7, "r2")
    out = np.zeros((128, 4), np.uint32)
    _check(lib().bn_rs_batch_table(_u32p(r2), _u32p(out)))
    return out


def rs_row_check(shat, r_low):
    """bn_rs_row_check: sum_v eq(r_low, v) s^_v; shat is (128, 4), r_low (7, 4). Host arithmetic."""
    shat, r_low = _rs_words(shat, 128, "shat"), _rs_words(r_low, 7, "r_low")
    out = np.zeros(4, np.uint32)
    _check(lib().bn_rs_row_check(_u32p(shat), _u32p(r_low), _u32p(out)))
    return out


def rs_sumcheck_claim(shat, r2):
    """bn_rs_sumcheck_claim: s_0 = sum_u B[u] s^row_u, the rows of s^ as a bit matrix. Host arithmetic."""
    shat, r2 = _rs_words(shat, 128, "shat"), _rs_words(r2, 7, "r2")
    out = np.zeros(4, np.uint32)
    _check(lib().bn_rs_sumcheck_claim(_u32p(shat), _u32p(r2), _u32p(out)))
    return out


def rs_eq_eval(r_high, rho, r2):
    """bn_rs_eq_eval: A~(rho), the mapped eq column of r_high at the sumcheck's challenges; r_high and
    rho are (n, 4), r2 (7, 4). Host arithmetic."""
    a = np.ascontiguousarray(r_high, dtype=np.uint32).reshape(-1, 4)
    b = np.ascontiguousarray(rho, dtype=np.uint32).reshape(-1, 4)
    if a.shape != b.shape:
        raise ValueError("the points differ in length")
    r2 = _rs_words(r2, 7, "r2")
    out = np.zeros(4, np.uint32)
    _check(lib().bn_rs_eq_eval(a.shape[0], _u32p(a) if len(a) else None, _u32p(b) if len(b) else None, _u32p(r2), _u32p(out)))
    return out


# ------------------------------------------------------------------ SHA-256 Merkle commitment
MERKLE_LEAF, MERKLE_ROW, MERKLE_TAIL = 0, 1, 2


def _merkle_size(fn, *args):
    n = ctypes.c_size_t()
    _check(fn(*args, ctypes.byref(n)))
    return n.value


def merkle_tree_digests(log_leaves):
    """bn_merkle_tree_digests: 2^(L+1) - 1, the 32-byte digests of the tree buffer."""
    return _merkle_size(lib().bn_merkle_tree_digests, log_leaves)


def merkle_row_offset(log_leaves, row):
    """bn_merkle_row_offset: the digest index of node 0 of `row` (row 0: the leaf digests; row L: the root)."""
    return _merkle_size(lib().bn_merkle_row_offset, log_leaves, row)


def merkle_open_bytes(log_leaves, log_leaf_elems):
    """bn_merkle_open_bytes: the bytes of one opening record, 16 * 2^a + 32 * L."""
    return _merkle_size(lib().bn_merkle_open_bytes, log_leaves, log_leaf_elems)


def _merkle_shape_ok(log_leaves, log_leaf_elems):
    return 0 <= log_leaf_elems <= 8 and 0 <= log_leaves and log_leaves + log_leaf_elems <= 30


def merkle_commit(data, log_leaves, log_leaf_elems, tree, stream=None, max_rows=0):
    """bn_merkle_commit_device: the SHA-256 Merkle tree of the 2^(L+a) compact elements in the device
    tensor `data` (leaf j: elements [j << a, (j + 1) << a)) into the device tensor `tree`
    (32 * (2^(L+1) - 1) bytes, row 0 first, the root last). Async on `stream` (default: torch's current
    stream of data's device); `data` is not written. max_rows != 0 forces the planner's rows-per-pass
    cap (bn_merkle_commit_device_split, a test hook)."""
    if _merkle_shape_ok(log_leaves, log_leaf_elems):  # else: the library's own error
        _check_device_tensor(data, 4 << (log_leaves + log_leaf_elems), "data")
        _check_device_tensor(tree, 8 * merkle_tree_digests(log_leaves), "tree")
    st = _stream(stream, _dev_index(data))
    if max_rows:
        _check(lib().bn_merkle_commit_device_split(_ptr(data), log_leaves, log_leaf_elems, _ptr(tree), max_rows, st))
    else:
        _check(lib().bn_merkle_commit_device(_ptr(data), log_leaves, log_leaf_elems, _ptr(tree), st))


def merkle_commit_host(data, log_leaf_elems, device=0):
    """bn_merkle_commit_host: the tree of a host array of 2^(L+a) elements ((n, 4) uint32), as a new
    (2^(L+1) - 1, 32) uint8 array; synchronous. L is taken from the array's size."""
    d = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1, 4)
    n = d.shape[0]
    if n == 0 or n & (n - 1) or not 0 <= log_leaf_elems <= 8 or n >> log_leaf_elems == 0:
        raise ValueError("data must hold a power of two of elements, at least one leaf")
    log_leaves = n.bit_length() - 1 - log_leaf_elems
    tree = np.zeros(((2 << log_leaves) - 1, 32), np.uint8)
    _check(lib().bn_merkle_commit_host(device, d.ctypes.data, log_leaves, log_leaf_elems, tree.ctypes.data))
    return tree


def merkle_open(data, tree, log_leaves, log_leaf_elems, indices, out, stream=None):
    """bn_merkle_open_device: the opening record of leaf indices[q] (the leaf's bytes, then the L
    sibling digests from the bottom up) at out + q * merkle_open_bytes(L, a). `indices` is a device
    tensor of 32-bit integers; an index >= 2^L gives an all-zero record. Async on `stream`."""
    nq = 0 if isinstance(indices, int) else indices.numel()
    if not isinstance(indices, int) and indices.element_size() != 4:
        raise ValueError("indices must be a tensor of 32-bit integers")
    if _merkle_shape_ok(log_leaves, log_leaf_elems):  # else: the library's own error
        _check_device_tensor(data, 4 << (log_leaves + log_leaf_elems), "data")
        _check_device_tensor(tree, 8 * merkle_tree_digests(log_leaves), "tree")
        _check_device_tensor(indices, nq, "indices")
        _check_device_tensor(out, nq * merkle_open_bytes(log_leaves, log_leaf_elems) // 4, "out")
    _check(lib().bn_merkle_open_device(_ptr(data), _ptr(tree), log_leaves, log_leaf_elems, _ptr(indices), nq, _ptr(out),
                                       _stream(stream, _dev_index(data))))


def _bytes32(b, what):
    a = np.frombuffer(bytes(b), dtype=np.uint8) if isinstance(b, (bytes, bytearray)) else np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
    if a.size != 32:
        raise ValueError("%s must be 32 bytes" % what)
    return np.ascontiguousarray(a)


def merkle_hash_leaf(leaf, log_leaf_elems):
    """bn_merkle_hash_leaf: the digest (32 bytes) of a leaf of 16 << a bytes (host arithmetic)."""
    a = np.frombuffer(bytes(leaf), dtype=np.uint8) if isinstance(leaf, (bytes, bytearray)) else np.ascontiguousarray(leaf).view(np.uint8).reshape(-1)
    if 0 <= log_leaf_elems <= 8 and a.size != 16 << log_leaf_elems:
        raise ValueError("the leaf holds %d bytes, need %d" % (a.size, 16 << log_leaf_elems))
    a = np.ascontiguousarray(a)
    out = np.zeros(32, np.uint8)
    _check(lib().bn_merkle_hash_leaf(a.ctypes.data, log_leaf_elems, out.ctypes.data))
    return out.tobytes()


def merkle_hash_node(left, right):
    """bn_merkle_hash_node: one compression of left || right from the initial state (host arithmetic)."""
    l, r = _bytes32(left, "left"), _bytes32(right, "right")
    out = np.zeros(32, np.uint8)
    _check(lib().bn_merkle_hash_node(l.ctypes.data, r.ctypes.data, out.ctypes.data))
    return out.tobytes()


def merkle_verify(root, log_leaves, log_leaf_elems, index, record):
    """bn_merkle_verify: True if the opening record of leaf `index` hashes to `root` (host arithmetic)."""
    rt = _bytes32(root, "root")
    rec = np.frombuffer(bytes(record), dtype=np.uint8) if isinstance(record, (bytes, bytearray)) else np.ascontiguousarray(record).view(np.uint8).reshape(-1)
    if _merkle_shape_ok(log_leaves, log_leaf_elems) and rec.size != merkle_open_bytes(log_leaves, log_leaf_elems):
        raise ValueError("the record holds %d bytes, need %d" % (rec.size, merkle_open_bytes(log_leaves, log_leaf_elems)))
    if index < 0:
        return False
    rec = np.ascontiguousarray(rec)
    ok = ctypes.c_int()
    _check(lib().bn_merkle_verify(rt.ctypes.data, log_leaves, log_leaf_elems, index, rec.ctypes.data, ctypes.byref(ok)))
    return bool(ok.value)


def merkle_commit_passes(log_leaves, log_leaf_elems, max_rows=0):
    """bn_merkle_commit_passes: the planner's passes as (kind, first row written, rows written), kind
    MERKLE_LEAF, MERKLE_ROW or MERKLE_TAIL (host only)."""
    out = (ctypes.c_int32 * 96)()
    n = ctypes.c_int()
    _check(lib().bn_merkle_commit_passes(log_leaves, log_leaf_elems, max_rows, out, 32, ctypes.byref(n)))
    return [(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(n.value)]
