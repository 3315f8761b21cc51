"""Multi-GPU sharding of chains: one process per GPU, no data-path collective, ONE all-gather of the draws.

Chains never interact during warm-up or sampling (everything in Driver.sample is per chain,
rainier-sampler/.../sampler/Driver.scala:13-17), so GPU g simply owns the global chains
[g*C, (g+1)*C) with seeds indexed by GLOBAL chain id -- results do not depend on the number of GPUs.
Observation columns and the compiled kernel are replicated per GPU.  The only exchange is the final
all-gather of the device-resident draws: RCCL over xGMI, issued by the engine itself behind the C ABI
(rh_comm_*, csrc/comm.cpp).  The host program only bootstraps it: rank 0's 128-byte RCCL unique id is
handed to the other ranks through whatever channel it has -- here a torch.distributed *gloo* (CPU)
broadcast, so that torch never initialises its own bundled HIP runtime next to the engine's.

(The single-process form -- one host thread per device inside one rh_sample_multi call -- is in sampler.sample_multi.)
"""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

from . import _capi


def shard_seeds(base_seed: int, chains_per_rank: int, rank: int) -> List[int]:
    """Seeds of the chains owned by `rank`: base + global chain id."""
    return [base_seed + rank * chains_per_rank + c for c in range(chains_per_rank)]


def global_chain_ids(chains_per_rank: int, rank: int) -> range:
    return range(rank * chains_per_rank, (rank + 1) * chains_per_rank)


def exchange_unique_id(dist, make_id, rank: int) -> bytes:
    """rank 0 creates the communicator id (make_id() -> 128 bytes), every rank receives it: a broadcast over the host
    program's own process group (gloo in bench.py and in the CPU test)."""
    box = [make_id() if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    assert isinstance(box[0], (bytes, bytearray)) and len(box[0]) == 128
    return bytes(box[0])


class Comm:
    """rh_comm: the RCCL communicator of one rank (include/rainier_hip.h, multi-process multi-GPU)."""

    def __init__(self, unique_id: bytes, world: int, rank: int, device: int):
        self.world, self.rank, self.device = world, rank, device
        self._h = C.c_void_p()
        _capi.check(_capi.lib().rh_comm_create(unique_id, world, rank, device, C.byref(self._h)))

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _capi.check(_capi.lib().rh_comm_unique_id(buf))
        return buf.raw

    def allgather_draws(self, sampler, to_host: bool = True):
        """every rank's draws [chains][iterations][nvars] -> [world*chains][iterations][nvars] (global chain id order);
        to_host = False leaves them on the device and returns the device pointer."""
        shape = (self.world * sampler.chains, sampler.iterations, sampler.model.nVars)
        if to_host:
            out = np.zeros(shape)
            _capi.check(_capi.lib().rh_comm_allgather_draws(self._h, sampler._h, _capi.dptr(out), None))
            return out
        p = C.c_void_p()
        _capi.check(_capi.lib().rh_comm_allgather_draws(self._h, sampler._h, None, C.byref(p)))
        return p.value

    def diagnostics(self, sampler, first: int = 0, count=None, moments: bool = False):
        """collective: Trace.diagnostics over the chains of ALL ranks -- one all-gather that stays on the device, analysed there
        (rh_diagnostics_device); every rank gets the same list of (rHat, effectiveSampleSize) as Sampler.diagnostics gives for its own"""
        from .sampler import diagnostics_device
        count = sampler.progress()[1] - int(first) if count is None else int(count)
        ptr = self.allgather_draws(sampler, to_host=False)
        return diagnostics_device(ptr, self.world * sampler.chains, sampler.iterations, sampler.model.nVars, device=self.device,
                                  first=first, count=count, moments=moments)

    def predict(self, sampler_or_gathered, predictor, first: int = 0, count=None, thin: int = 1, to_host: bool = True,
                diagnostics: bool = False, chains: int = None, iterations: int = None, nvars: int = None):
        """collective (when given a sampler): Trace.predict over the chains of ALL ranks -- one all-gather that stays on the device,
        evaluated there (rh_predict_device).  sampler_or_gathered: a Sampler, or the device pointer allgather_draws(to_host=False)
        returned together with chains (world * per rank) / iterations / nvars."""
        from .sampler import predict_device
        if isinstance(sampler_or_gathered, int):
            ptr = sampler_or_gathered
            count = int(iterations) - int(first) if count is None else int(count)
        else:
            s = sampler_or_gathered
            chains, iterations, nvars = self.world * s.chains, s.iterations, s.model.nVars
            count = s.progress()[1] - int(first) if count is None else int(count)
            ptr = self.allgather_draws(s, to_host=False)
        return predict_device(predictor, ptr, chains, iterations, nvars, device=self.device, first=first, count=count, thin=thin,
                              to_host=to_host, diagnostics=diagnostics)

    def summary(self, sampler, first: int = 0, count=None, thin: int = 1, probs=(0.055, 0.945), hdpi=0.89):
        """collective: precis' figures and hdpi over the chains of ALL ranks -- one all-gather that stays on the device, sorted and
        summarised there (rh_summary_device); every rank gets the same Summary as Sampler.summary gives for its own chains"""
        from .sampler import summary_device
        count = sampler.progress()[1] - int(first) if count is None else int(count)
        ptr = self.allgather_draws(sampler, to_host=False)
        return summary_device(ptr, self.world * sampler.chains, sampler.iterations, sampler.model.nVars, device=self.device,
                              first=first, count=count, thin=thin, probs=probs, hdpi=hdpi)

    def allreduce_max(self, v: float) -> float:
        a = np.array([float(v)])
        _capi.check(_capi.lib().rh_comm_allreduce_max(self._h, _capi.dptr(a)))
        return float(a[0])

    def close(self):
        if self._h:
            _capi.lib().rh_comm_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


def device_synchronize(device: int) -> None:
    _capi.check(_capi.lib().rh_device_synchronize(int(device)))
