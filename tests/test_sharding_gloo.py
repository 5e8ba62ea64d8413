"""gloo tests (CPU) of the multi-GPU exchange logic (kzg_snark_amd/sharding.py, plonk_sharded.py) at world sizes
2, 3, 4 and 8 -- eight being the machine's.  The per-rank commit, transform and opening are the oracle's (Python ints,
tests/oracle_backends.py) standing in for the engine: the exchanges (round-robin ownership, all-gathers, the
all-to-alls of the four-step transforms, carries, the quotient's re-partition) and the index arithmetic that depends on
the world size are what is under test."""
import os
import random
import socket

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import py_oracle as O


import datetime

_PG_TIMEOUT = datetime.timedelta(seconds=240)        # a rank whose peer died gives up instead of waiting half an hour


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(target, world, timeout, extra=()):
    """Spawn `world` ranks of `target(rank, world, port, queue, *extra)` and collect one result each.  Whatever goes
    wrong -- a rank that raised leaves its peers blocked in a gloo collective, a queue that stays empty -- every
    child is terminated (then killed) before the error travels on: no process is left holding the GPU or the port,
    and pytest does not hang joining non-daemon children."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q, *extra)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = []
        for _ in range(world):
            res.append(q.get(timeout=timeout))
            if res[-1][1] != "ok":                      # its peers may never return from their collective
                break
        for p in procs:
            p.join(timeout=60 if len(res) == world and all(v == "ok" for _, v in res) else 1)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()
    return res


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=_PG_TIMEOUT)
    try:
        from kzg_snark_amd import curve as C
        from kzg_snark_amd.sharding import DistributedCommitter, range_of
        cv = O.BN254
        G = C.g1_group(C.CURVES["bn254"])
        tau = 0xabcdef
        n = 13
        full_ck = O.setup(n - 1, tau, cv)
        rng = random.Random(5)
        polys = [[rng.randrange(cv.r) for _ in range(rng.randrange(1, n + 1))] for _ in range(4)] + [[0, 0]]

        def to_pt(p):
            a = O.normalize(p, cv)
            return (1, 1, 0) if a is None else (a[0], a[1], 1)

        # batch mode: replicated key, polynomials dealt round-robin
        dc = DistributedCommitter(lambda ps: [to_pt(c) for c in O.commit(full_ck, ps, cv)], G.add, G.Z)
        got = dc.commit_batch(polys)
        want = [to_pt(c) for c in O.commit(full_ck, polys, cv)]
        assert got == want, "batch mode"

        # range mode: key and coefficients sharded by contiguous range
        lo, hi = range_of(rank, world, n)
        shard_ck = full_ck[lo:hi]
        p = [rng.randrange(cv.r) for _ in range(n)]
        dc2 = DistributedCommitter(lambda ps: [to_pt(c) for c in O.commit(shard_ck, ps, cv)], G.add, G.Z)
        got = dc2.commit_range(p[lo:hi])
        assert got == to_pt(O.commit(full_ck, [p], cv)[0]), "range mode"
        # the same with the partial points added by the library's host group law (kzg_g1_sum) instead of one by one
        from kzg_snark_amd import _native
        dc3 = DistributedCommitter(lambda ps: [to_pt(c) for c in O.commit(shard_ck, ps, cv)], G.add, G.Z,
                                   sum_fn=lambda pts: _native.g1_sum("bn254", pts))
        assert dc3.commit_range(p[lo:hi]) == got, "range mode, sum_fn"
        assert got == to_pt(O.commit_trapdoor(p, tau, cv))

        # range-mode open: slice evaluation, carry exchange, quotient slice against a key shard that
        # starts at lo - 1 (the oracle stands in for kzg_open_shard_begin / _finish)
        r = cv.r
        polys3 = [[rng.randrange(r) for _ in range(m)] for m in (n, 9, 4)]
        z, xi = rng.randrange(r), rng.randrange(r)
        comb = O.combine(polys3, xi, r) + [0] * n
        comb = comb[:n]
        local = comb[lo:hi]

        def begin():
            return O.poly_eval(local, z, r)

        def finish(carry, first):
            ext = local + [carry]
            S = [0] * (len(ext) + 1)
            for j in range(len(ext) - 1, -1, -1):
                S[j] = (ext[j] + z * S[j + 1]) % r
            if first:
                vec, start, ev = S[1:len(local)], 0, S[0]
            else:
                vec, start, ev = S[0:len(local)], lo - 1, None
            key = full_ck[start:start + len(vec)]
            return to_pt(O.commit(key, [vec], cv)[0]) if vec else (1, 1, 0), ev

        proof, ev = dc2.open_range(begin, finish, z, r, n)
        want, pz = O.open_(full_ck, polys3, z, xi, cv)
        assert proof == to_pt(want) and ev == pz, "range-mode open"

        # the fused step (one polynomial committed and k opened, two exchanges): same results
        box = {}
        com, (proof2, ev2) = dc2.commit_and_open_range(
            lambda: box.setdefault("c", to_pt(O.commit(shard_ck, [p[lo:hi]], cv)[0])), lambda: box["c"],
            begin, finish, z, r, n)
        assert com == to_pt(O.commit(full_ck, [p], cv)[0]) and proof2 == proof and ev2 == ev, "fused range step"
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def _oracle_backends():
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import oracle_backends
    return oracle_backends


def _ntt_worker(rank, world, port, q, log_n=7):
    import numpy as np
    import torch
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=_PG_TIMEOUT)
    try:
        from kzg_snark_amd.sharding import DistributedNTT
        cv = O.BLS12_381
        n = 1 << log_n
        rng = random.Random(99)
        x = [rng.randrange(cv.r) for _ in range(n)]
        for w, inverse in ((cv.root_of_unity(n), False), (cv.root_of_unity(n), True), (rng.randrange(2, cv.r), False)):
            want = O.ifft_ff(x, w, cv.r) if inverse else O.fft_ff(x, w, cv.r)
            lo, hi = rank * n // world, (rank + 1) * n // world
            buf = b"".join(v.to_bytes(32, "little") for v in x[lo:hi])
            xl = torch.from_numpy(np.frombuffer(buf, dtype="<i8").reshape(hi - lo, 4).copy())
            OB = _oracle_backends()
            d = DistributedNTT(OB.OracleNttOps(log_n, w, cv.r, inverse))
            got = OB.ints_of(d.transform(xl.clone(), log_n))
            assert got == want[lo:hi], (inverse, "distributed NTT shard mismatch")
            # two all-to-alls: the result stays in the row pass's order
            from kzg_snark_amd.sharding import transposed_index
            got_t = OB.ints_of(d.transform(xl.clone(), log_n, layout="transposed"))
            assert got_t == [want[transposed_index(log_n, world, rank, i)] for i in range(hi - lo)], "transposed layout"
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_two_rank_distributed_ntt():
    """The all-to-all choreography of the multi-GPU four-step NTT (natural order in; natural order
    out with three exchanges or the transposed layout with two; arbitrary w, inverse) with the
    oracle as the local transform."""
    res = _run_ranks(_ntt_worker, 2, 180)
    assert sorted(res) == [(0, "ok"), (1, "ok")], res


@pytest.mark.parametrize("log_n", [6, 7])
def test_eight_rank_distributed_ntt(log_n):
    """The same at the machine's world size.  2^6 over eight ranks is the degenerate split (N1 = N2 = 8: every rank
    holds ONE row and ONE column, R1 = W = 1), 2^7 the odd one (N1 = 16, N2 = 8: two rows, one column)."""
    res = _run_ranks(_ntt_worker, 8, 180, (log_n,))
    assert sorted(res) == [(r, "ok") for r in range(8)], res


def test_two_rank_exchange():
    res = _run_ranks(_worker, 2, 120)
    assert sorted(res) == [(0, "ok"), (1, "ok")], res


def test_range_partition():
    from kzg_snark_amd.sharding import range_of, round_robin
    for n in (1, 7, 8, 1 << 20, (1 << 20) + 6):
        for world in (1, 2, 3, 8):
            parts = [range_of(r, world, n) for r in range(world)]
            assert parts[0][0] == 0 and parts[-1][1] == n
            assert all(parts[i][1] == parts[i + 1][0] for i in range(world - 1))
            assert max(h - l for l, h in parts) - min(h - l for l, h in parts) <= 1
    assert round_robin(5, 2) == [0, 1, 0, 1, 0]


def _golden(name):
    import json
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)))


def _check_frozen_proof(proof, gp):
    """proof dict == tests/golden/plonk_proof_n16.json, bit for bit"""
    want = gp["proof"]
    for k, v in want["commitments"].items():
        assert tuple(int(c) for c in proof["commitments"][k]) == (int(v[0], 16), int(v[1], 16), v[2]), k
    for k, v in want["evaluations"].items():
        assert int(proof["evaluations"][k]) == int(v, 16), k
    for k, v in want["kzg_proofs"].items():
        assert tuple(int(c) for c in proof["kzg_proofs"][k]) == (int(v[0], 16), int(v[1], 16), v[2]), k


def _plonk_worker(rank, world, port, q, device):
    """One rank of a PLONK proof dealt over `world` ranks (sharding.ProofSharding; BASELINE config 5 on several
    GPUs).  device=False: host prover, the oracle standing in for the engine's commit / open / INTT (CPU);
    device=True: the device prover on cuda:0 (every rank on the test box's one GPU)."""
    import sys
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=_PG_TIMEOUT)
    try:
        here = os.path.dirname(os.path.abspath(__file__))
        if here not in sys.path:
            sys.path.insert(0, here)
        import test_plonk as TP
        from kzg_snark_amd import plonk
        from kzg_snark_amd.sharding import ProofSharding
        gp = _golden("plonk_proof_n16.json")
        circuit = TP.fixture_instance()
        curve, tau = gp["curve"], int(gp["tau"], 16)
        blinders = [int(v, 16) for v in gp["blinders"]]
        if not device:
            from kzg_snark_amd.field import PolynomialRing
            plonk.fft_ff_interpolation = lambda values, g, F: PolynomialRing(F, "X")(
                O.fft_ff_interpolation([int(v) for v in values], int(g), F.p))
            sh = ProofSharding()
            idx, prv = plonk.Indexer(curve), plonk.Prover(curve, sharding=sh)
            idx.kzg = prv.kzg = TP.oracle_backed(curve)
            ipk, ivk = idx.preprocess(*circuit[:6], tau=tau)
            # only rank 0's blinders count: the others pass different ones and must end with the same proof
            mine = blinders if rank == 0 else [b + 1 + rank for b in blinders]
            proof = prv.prove(ipk, circuit[6], circuit[7], blinders=mine)
            _check_frozen_proof(proof, gp)
            assert sh.exchanges == 1 + 3 + 1, sh.exchanges        # blinders, three rounds of commitments, the openings
        else:
            from kzg_snark_amd import plonk_device
            idx = plonk_device.DeviceIndexer(curve)
            ipk, ivk = idx.preprocess(*circuit[:6], tau=tau)
            for deal in (False, True):
                sh = ProofSharding(deal_transforms=deal)
                prv = plonk_device.DeviceProver(curve, alg=idx.alg, sharding=sh)
                mine = blinders if rank == 0 else [b + 1 + rank for b in blinders]
                proof = prv.prove(ipk, circuit[6], circuit[7], blinders=mine)
                _check_frozen_proof(proof, gp)
                assert sh.exchanges == 5 + (8 if deal else 0), (deal, sh.exchanges)
                assert plonk.Verifier(curve).verify(ivk, circuit[6], proof)
            # a larger synthetic circuit: all ranks end with the same proof, and the verifier accepts it
            from kzg_snark_amd.field import GF
            F = GF(O.BLS12_381.r)
            big = plonk.synthetic_circuit(1 << 12, F, seed=12)
            idx2 = plonk_device.DeviceIndexer("bls12_381")
            ipk2, ivk2 = idx2.preprocess(*big[:6], tau=0x1234567)
            sh = ProofSharding()
            prv2 = plonk_device.DeviceProver("bls12_381", alg=idx2.alg, sharding=sh)
            proof2 = prv2.prove(ipk2, big[6], big[7])                          # random blinders: rank 0's are shared
            assert plonk.Verifier("bls12_381").verify(ivk2, big[6], proof2)
            import hashlib
            digest = hashlib.sha256(repr(sorted((k, tuple(int(c) for c in v)) for k, v in
                                                list(proof2["commitments"].items())
                                                + list(proof2["kzg_proofs"].items()))).encode()).digest()
            from kzg_snark_amd.sharding import all_gather_bytes
            assert len(set(all_gather_bytes(digest))) == 1, "ranks ended with different proofs"
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _run_plonk_ranks(world, device, timeout):
    res = _run_ranks(_plonk_worker, world, timeout, (device,))
    assert sorted(res) == [(r, "ok") for r in range(world)], res


def _sharded_ipk(ipk, OB):
    """proving key of the host indexer -> the tensors the vector-sharded prover slices (what DeviceIndexer leaves on
    the device: coefficient vectors of the eight preprocessed polynomials, sigma* values)"""
    n = ipk["subgroups"]["n"]
    co = {k: OB.tensor_of(([int(c) for c in p.list()] + [0] * n)[:n]) for k, p in ipk["polynomials"].items()}
    ss = ipk["sigma_star"]
    sv = {f"S_sigma{b + 1}": OB.tensor_of([int(v) for v in ss[b * n:(b + 1) * n]]) for b in range(3)}
    return {"ck": ipk["ck"], "coeffs": co, "sigma_values": sv, "subgroups": ipk["subgroups"]}


def _proof_key(proof):
    return (sorted((k, tuple(int(c) for c in v)) for k, v in list(proof["commitments"].items())
                   + list(proof["kzg_proofs"].items())),
            sorted((k, int(v)) for k, v in proof["evaluations"].items()))


def _digests_agree(proof):
    """every rank's proof -- commitments, openings AND evaluations -- through one all-gather of a SHA-256"""
    import hashlib
    from kzg_snark_amd.sharding import all_gather_bytes
    digests = all_gather_bytes(hashlib.sha256(repr(_proof_key(proof)).encode()).digest())
    assert len(set(digests)) == 1, "ranks ended with different proofs"


def _sharded_worker(rank, world, port, q, case, gates=64):
    """One rank of a PLONK proof whose VECTORS are split over `world` ranks (plonk_sharded.ShardedProver), the oracle
    standing in for the engine (tests/oracle_backends.py): distributed INTTs and coset NTTs through the all-to-alls,
    accumulator carries, quotient re-partition, range-sharded commitments and openings."""
    import sys
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=_PG_TIMEOUT)
    try:
        OB = _oracle_backends()
        import test_plonk as TP
        from kzg_snark_amd import plonk, plonk_sharded
        from kzg_snark_amd.field import GF, PolynomialRing
        plonk.fft_ff_interpolation = lambda values, g, F: PolynomialRing(F, "X")(
            O.fft_ff_interpolation([int(v) for v in values], int(g), F.p))
        if case == "frozen":
            gp = _golden("plonk_proof_n16.json")
            circuit, curve, tau = TP.fixture_instance(), gp["curve"], int(gp["tau"], 16)
            blinders = [int(v, 16) for v in gp["blinders"]]
        else:
            curve, tau = "bn254", 0x7a75
            circuit = plonk.synthetic_circuit(gates, GF(O.curve(curve).r), seed=3)
            blinders = list(range(101, 112))
        mine = blinders if rank == 0 else [b + 1 + rank for b in blinders]       # only rank 0's count
        if world == 8:
            # 64 gates pass the guard this prover used to have (n / G >= 8) and are one size too small for eight ranks:
            # refused by every rank BEFORE the first exchange, so the group is as it was -- the proof below runs
            # through it
            assert gates == 128
            small = plonk.synthetic_circuit(gates // 2, GF(O.curve(curve).r), seed=3)
            idx0 = plonk.Indexer(curve)
            idx0.kzg = TP.oracle_backed(curve)
            ipk0, _ = idx0.preprocess(*small[:6], tau=tau)
            sp0 = plonk_sharded.ShardedProver(curve, OB.OracleShardBackend(curve))
            with pytest.raises(ValueError, match=rf"smallest n for {world} ranks is {gates}\b"):
                sp0.prove(_sharded_ipk(ipk0, OB), small[6], small[7], blinders=mine)
            assert sp0.exchanges == 0 and sp0.tf.exchanges == 0
        idx = plonk.Indexer(curve)
        idx.kzg = TP.oracle_backed(curve)
        ipk, ivk = idx.preprocess(*circuit[:6], tau=tau)
        sp = plonk_sharded.ShardedProver(curve, OB.OracleShardBackend(curve))
        proof = sp.prove(_sharded_ipk(ipk, OB), circuit[6], circuit[7], blinders=mine)
        _digests_agree(proof)
        if case == "frozen":
            _check_frozen_proof(proof, gp)
        elif world < 8 or rank == 0:
            # the unsharded host prover with the same blinders: the same proof, and the verifier accepts it (at eight
            # ranks on rank 0 alone: the digest above ties the other seven to it)
            ref = plonk.Prover(curve)
            ref.kzg = TP.oracle_backed(curve)
            want = ref.prove(ipk, circuit[6], circuit[7], blinders=blinders)
            assert _proof_key(proof) == _proof_key(want)
            if rank == 0:
                ver = plonk.Verifier(curve)
                assert ver.verify(ivk, circuit[6], proof)
        assert sp.tf.exchanges > 0 and sp.exchanges > 0
        q.put((rank, "ok"))
    except BaseException as e:  # noqa: BLE001  (pytest.raises fails with a BaseException)
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,case,gates", [
    pytest.param(2, "frozen", 16, id="2-frozen"), pytest.param(2, "synthetic", 64, id="2-synthetic"),
    pytest.param(4, "synthetic", 64, id="4-synthetic"), pytest.param(8, "synthetic", 128, id="8-synthetic-128")])
def test_vector_sharded_proof_over_ranks(world, case, gates):
    """BASELINE config 5 with the vector work split over the ranks (plonk/prover.py:83-85, 243-264, 297-316 on range /
    transposed shards; commitments and openings against key shards): two ranks reproduce
    tests/golden/plonk_proof_n16.json bit for bit (n = 16 leaves a rank the minimum of 8 rows); two, four and eight
    ranks reproduce the unsharded host prover's proof of a 64-gate (eight ranks: 128-gate) circuit, which the verifier
    accepts, and every rank ends with the same proof.  128 gates is the least eight ranks can split
    (plonk_sharded.can_shard_vectors): the 64-gate circuit is refused first, with no exchange issued, and the proof
    then runs through the same process group.  At eight ranks the quotient's re-partition takes its one-slot form
    (plonk_sharded._split_quotient: cap = 1, the tail on rank 6, ranks 6 and 7 sending nothing)."""
    res = _run_ranks(_sharded_worker, world, 600, (case, gates))
    assert sorted(res) == [(r, "ok") for r in range(world)], res


def test_which_sizes_can_be_vector_sharded():
    """plonk_sharded.can_shard_vectors against what each transform of the prover asks for, stated directly: a rank's
    range of at least 8 coefficients; ShardedTransforms.t_index: G | N1; T_shift by the four rows of z(g X):
    4 <= R1 = N1 / G -- N1 the row count of the 4n-point four-step matrix, here the least power of two whose square
    reaches 4n.  min_sharded_gates is the least accepted power of two."""
    from kzg_snark_amd import plonk_sharded
    table = {}
    for log_n in range(3, 13):
        n = 1 << log_n
        N1 = 1
        while N1 * N1 < 4 * n:
            N1 *= 2
        for G in (1, 2, 4, 8, 16):
            need = n % G == 0 and n // G >= 8 and N1 % G == 0 and 0 < 4 <= N1 // G
            table[n, G] = need
            assert plonk_sharded.can_shard_vectors(n, G) == need, (n, G)
    for G in (1, 2, 4, 8, 16):
        least = min(n for (n, g), ok in table.items() if g == G and ok)
        assert plonk_sharded.min_sharded_gates(G) == least, G
        assert all(table[n, G] for n in (1 << k for k in range(3, 13)) if n >= least), G     # monotone above it
    assert [plonk_sharded.min_sharded_gates(G) for G in (1, 2, 4, 8, 16)] == [8, 16, 32, 128, 512]
    assert table[64, 8] is False and table[256, 16] is False          # the old guard (n / G >= 8 alone) let these in
    for G in (0, 3, 6, 12):
        assert not plonk_sharded.can_shard_vectors(1 << 12, G), G
    assert not plonk_sharded.can_shard_vectors(24 * 8 + 4, 8)          # G does not divide n


def _transforms_worker(rank, world, port, q):
    """sharding.ShardedTransforms, each method on its own against the oracle's whole transform (Python ints)."""
    import torch
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=_PG_TIMEOUT)
    try:
        OB = _oracle_backends()
        from kzg_snark_amd.sharding import ShardedTransforms, transposed_index
        cv = O.BLS12_381
        r, G, g = cv.r, world, rank
        be = OB.OracleShardBackend("bls12_381")
        tf = ShardedTransforms(be.ntt_ops, be.full_ntt, min_log=2)
        rng = random.Random(4242)                         # the same vectors on every rank

        def vector(n):
            v = [rng.randrange(r) for _ in range(n)]
            v[0], v[-1] = r - 1, 0
            return v

        def did(count, what):
            """the transform just run issued `count` exchanges"""
            nonlocal seen
            assert tf.exchanges - seen == count, (what, tf.exchanges - seen, count)
            seen = tf.exchanges

        seen = 0
        padded_branches = set()
        for log_n in (6, 7, 8, 9):
            n = 1 << log_n
            m = n // G
            lo, hi = g * m, (g + 1) * m
            w = cv.root_of_unity(n)
            # natural_batch: three vectors through ONE set of all-to-alls (the stacked exchange)
            xs = [vector(n) for _ in range(3)]
            for inverse in (False, True):
                got = tf.natural_batch([OB.tensor_of(x[lo:hi]) for x in xs], log_n, w, inverse)
                did(3, "natural_batch")
                for x, t in zip(xs, got):
                    want = O.ifft_ff(x, w, r) if inverse else O.fft_ff(x, w, r)
                    assert OB.ints_of(t) == want[lo:hi], ("natural_batch", log_n, inverse)
            # T_to_natural: this rank's shard of the transposed layout in, its contiguous range out
            x = xs[0]
            xT = OB.tensor_of([x[transposed_index(log_n, G, g, i)] for i in range(m)])
            for inverse in (False, True):
                keep = xT.clone()
                got = tf.T_to_natural(xT, log_n, w, inverse)
                did(2, "T_to_natural")
                want = O.ifft_ff(x, w, r) if inverse else O.fft_ff(x, w, r)
                assert OB.ints_of(got) == want[lo:hi], ("T_to_natural", log_n, inverse)
                assert torch.equal(xT, keep), "T_to_natural must leave its input alone"
            # padded_to_T_batch: n coefficients of a zero-padded 4n vector -> its transform in the transposed layout
            log_big = log_n + 2
            big = 4 * n
            w_big = cv.root_of_unity(big)
            kb = (log_big + 1) // 2
            N1b, N2b = 1 << kb, 1 << (log_big - kb)
            R1b = N1b // G
            got = tf.padded_to_T_batch([OB.tensor_of(x[lo:hi]) for x in xs[:2]], log_n, log_big, w_big)
            two_exchanges = m % N2b == 0            # whole rows of the big matrix per rank; else gather and transform
            did(2 if two_exchanges else 1, ("padded_to_T_batch", log_n))
            padded_branches.add(two_exchanges)
            for x, t in zip(xs[:2], got):
                want = O.fft_ff(x + [0] * (big - n), w_big, r)
                assert OB.ints_of(t) == [want[transposed_index(log_big, G, g, i)] for i in range(big // G)], \
                    ("padded_to_T_batch", log_n)
            # T_shift: y[i] = full[(i + s) mod 4n] in the transposed layout; the last rank's rows wrap into the next b
            full = vector(big)
            idx = [transposed_index(log_big, G, g, i) for i in range(big // G)]
            assert idx == [int(v) for v in tf.t_index(log_big, "cpu")]
            fT = OB.tensor_of([full[i] for i in idx])
            for s in sorted({1, 4, R1b} - ({4} if R1b < 4 else set())):
                got = tf.T_shift(fT, log_big, s)
                did(1, "T_shift")
                assert OB.ints_of(got) == [full[(i + s) % big] for i in idx], ("T_shift", log_n, s)
            for s in (0, R1b + 1):
                with pytest.raises(ValueError):
                    tf.T_shift(fT, log_big, s)
                did(0, "T_shift refusing")
        want_branches = {True, False} if G == 8 else {True}         # 2^6 over eight ranks: m = 8 < N2' = 16
        assert padded_branches == want_branches, padded_branches
        q.put((rank, "ok"))
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_transforms_over_ranks(world):
    """The four transforms of the vector-sharded prover called directly, 2^6 .. 2^9 elements over 2, 4 and 8 ranks,
    every output element against the oracle's fft_ff / ifft_ff of the whole vector: natural_batch (three vectors, one
    set of all-to-alls), T_to_natural, padded_to_T_batch into a 4n-point domain -- the two-exchange path, and at eight
    ranks and 2^6 the gather fallback, told apart by the exchange count -- and T_shift by 1, 4 and a rank's whole row
    count, whose last rank wraps around; shifts of 0 and of more than a rank's rows are refused."""
    res = _run_ranks(_transforms_worker, world, 300)
    assert sorted(res) == [(r, "ok") for r in range(world)], res


def test_vector_sharding_needs_a_power_of_two_world():
    """Three ranks cannot split the radix-2 transforms: make_prover then keeps the dealt-MSM prover (the world-size-3
    test below), and hands out the vector-sharded one for 1, 2, 4, 8 ranks."""
    from types import SimpleNamespace
    from kzg_snark_amd import plonk_sharded
    alg = SimpleNamespace(ctx=None, r=O.BN254.r)
    for world, want in ((1, "ShardedProver"), (2, "ShardedProver"), (3, "DeviceProver"), (4, "ShardedProver"),
                        (6, "DeviceProver"), (8, "ShardedProver")):
        sh = SimpleNamespace(world=world, shard_vectors=True, group=None)
        assert type(plonk_sharded.make_prover("bn254", alg, sh)).__name__ == want, world
    sh = SimpleNamespace(world=4, shard_vectors=False, group=None)
    assert type(plonk_sharded.make_prover("bn254", alg, sh)).__name__ == "DeviceProver"


@pytest.mark.parametrize("world", [2, 3])
def test_plonk_proof_dealt_over_ranks_is_the_frozen_proof(world):
    """BASELINE config 5 across ranks (plonk/prover.py:89,113,136,184-185 dealt by sharding.ProofSharding): the
    reference's 16-gate instance proved by 2 and by 3 ranks -- commitments of a round round-robin, one opening per
    rank, blinders from rank 0 -- reproduces tests/golden/plonk_proof_n16.json bit for bit on every rank."""
    _run_plonk_ranks(world, device=False, timeout=300)


def _sharded_gpu_worker(rank, world, port, q, parts=("frozen", 12, 13)):
    """The vector-sharded prover on the engine (plonk_sharded.GpuShardBackend), `world` ranks sharing the test box's
    GPU over gloo (tensors make the round trip through the host in the exchanges).  parts: "frozen" = the 16-gate
    instance, 12 / 13 = the synthetic proofs of 2^12 / 2^13 gates."""
    import hashlib
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=_PG_TIMEOUT)
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        if here not in sys.path:
            sys.path.insert(0, here)
        import test_plonk as TP
        from kzg_snark_amd import plonk, plonk_device, plonk_sharded
        from kzg_snark_amd.field import GF
        from kzg_snark_amd.sharding import ProofSharding, all_gather_bytes
        if "frozen" in parts:
            # 1. the frozen 16-gate proof (every transform below the distributed sizes: gather, transform, keep a share)
            gp = _golden("plonk_proof_n16.json")
            circuit = TP.fixture_instance()
            curve, tau = gp["curve"], int(gp["tau"], 16)
            blinders = [int(v, 16) for v in gp["blinders"]]
            idx = plonk_device.DeviceIndexer(curve)
            ipk, ivk = idx.preprocess(*circuit[:6], tau=tau)
            prv = plonk_sharded.make_prover(curve, idx.alg, ProofSharding(shard_vectors=True))
            assert type(prv).__name__ == "ShardedProver"
            mine = blinders if rank == 0 else [b + 1 + rank for b in blinders]
            proof = prv.prove(ipk, circuit[6], circuit[7], blinders=mine)
            _check_frozen_proof(proof, gp)
            assert plonk.Verifier(curve).verify(ivk, circuit[6], proof)
        # 2. 2^12 and 2^13 gates on BLS12-381: the 4n-point (and at 2^13 the n-point) transforms go through the
        # all-to-alls and the device's column / row passes; same blinders as the unsharded device prover -> the same
        # proof on every rank, and the verifier accepts it
        F = GF(O.BLS12_381.r)
        for log_gates in (p for p in parts if p != "frozen"):
            big = plonk.synthetic_circuit(1 << log_gates, F, seed=log_gates)
            idx2 = plonk_device.DeviceIndexer("bls12_381")
            ipk2, ivk2 = idx2.preprocess(*big[:6], tau=0x1234567)
            bl = list(range(7, 18))
            want = plonk_device.DeviceProver("bls12_381", alg=idx2.alg).prove(ipk2, big[6], big[7], blinders=bl)
            sp = plonk_sharded.make_prover("bls12_381", idx2.alg, ProofSharding(shard_vectors=True))
            got = sp.prove(ipk2, big[6], big[7], blinders=bl if rank == 0 else [1] * 11)
            assert _proof_key(got) == _proof_key(want), log_gates
            assert plonk.Verifier("bls12_381").verify(ivk2, big[6], got)
            digest = hashlib.sha256(repr(_proof_key(got)).encode()).digest()
            assert len(set(all_gather_bytes(digest))) == 1, "ranks ended with different proofs"
            # per proof 3 + 2 (round 1, batched), 3 + 2 + 1 (round 2), 4 + 1 (round 3); + 2 once for the circuit cosets
            assert 0 < sp.tf.exchanges <= 18
            del ipk2, sp, idx2
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 8])
def test_vector_sharded_device_prover_on_one_gpu(world):
    """plonk_sharded.ShardedProver on the engine: one rank (every exchange degenerate, the shard logic alone) and two
    ranks sharing the GPU over gloo.  The frozen 16-gate proof bit for bit; 2^12- and 2^13-gate proofs identical to
    the unsharded device prover's for the same blinders, accepted by the verifier, the same on every rank.
    Eight ranks -- the machine's world size, eight processes on the one GPU -- prove the 2^13 gates only: the least size
    at which both the n-point and the 4n-point transforms take the distributed passes (8 and 16 columns and rows of
    them per rank), and the frozen 16 gates cannot be split eight ways (plonk_sharded.can_shard_vectors)."""
    parts = (13,) if world == 8 else ("frozen", 12, 13)
    res = _run_ranks(_sharded_gpu_worker, world, 900, (parts,))
    assert sorted(res) == [(r, "ok") for r in range(world)], res


@pytest.mark.gpu
def test_device_prover_dealt_over_two_ranks_on_one_gpu():
    """The same with the device prover (kzg_snark_amd/plonk_device.py), two ranks sharing the test box's GPU over
    gloo: the frozen 16-gate proof bit for bit with replicated and with dealt transforms, and a 2^12-gate
    BLS12-381 proof that every rank ends with identically and the host verifier accepts."""
    _run_plonk_ranks(2, device=True, timeout=600)
