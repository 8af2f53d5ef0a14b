"""TEST INFRASTRUCTURE ONLY: restatements of srslte_phich_decode / srslte_phich_calc (lib/src/phy/phch/phich.c:133-315),
of dci_format0_pack / dci_format0_unpack (phch/dci.c:416-574) and of the UE blind search with its pending UL list
(ue/ue_dl.c:420-641), built from pieces that are pinned elsewhere:

  oracle.pdcch_chain.regs   the PHICH REG map: the reference's own srslte_regs_init where oracle/_ref is built
                            (use_ref=True), else the orc_ restatement the PDCCH tests pin against it
  orc_ctrl_equalize         the control-channel equalisers (liboracle.so)
  oracle.sequence_lte       the Gold sequence

The despreading, the BPSK demapper and srslte_phich_ack_decode are written here in numpy float32, in the reference's
order of operations."""
from __future__ import annotations

import numpy as np

import oracle
from oracle import pdcch_chain as pd

NSF, NSEQ, NBITS, NSYM = 4, 8, 3, 12
PHICH_RES = {0: 1 / 6, 1: 1 / 2, 2: 1.0, 3: 2.0}
# 36.211 Table 6.9.1-2 (phich.c:40-47)
W_NORMAL = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1],
                     [1j, 1j, 1j, 1j], [1j, -1j, 1j, -1j], [1j, 1j, -1j, -1j], [1j, -1j, -1j, 1j]], np.complex64)
f32 = np.float32


def regs(nof_prb, nof_ports, cell_id, phich_res, phich_ext):
    return pd.regs(nof_prb, nof_ports, cell_id, phich_res, phich_ext, 1, use_ref=oracle.ref_available())


def ngroups_formula(nof_prb, phich_res):
    """36.211 6.9: ceil(Ng * (N_RB / 8)) in float as regs.c computes it."""
    return int(np.ceil(f32(PHICH_RES[phich_res]) * (f32(nof_prb) / f32(8))))


def phich_calc(ngroups, n_prb_lowest, n_dmrs, I_phich):
    """phich.c:138-139"""
    return (n_prb_lowest + n_dmrs) % ngroups + I_phich * ngroups, ((n_prb_lowest // ngroups) + n_dmrs) % (2 * NSF)


def seq_float(cell_id, sf_idx):
    c = oracle.sequence_lte((sf_idx + 1) * (2 * cell_id + 1) * 512 + cell_id, NSYM)  # sequences.c:45-48, nslot = 2 sf
    return np.where(c != 0, -1.0, 1.0).astype(f32)


def phich_decode(grids, ce, re12, cell_id, sf_idx, nseq, noise):
    """srslte_phich_decode for one resource.  grids (rx, G), ce (ports, rx, G) complex64, re12 the group's REs.
    Returns (ack_value, distance); distance None when srslte_phich_ack_decode leaves it unwritten."""
    grids = np.ascontiguousarray(grids, np.complex64)
    ce = np.ascontiguousarray(ce, np.complex64)
    nports, nrx = ce.shape[0], grids.shape[0]
    y = np.ascontiguousarray(grids[:, re12])
    h = np.ascontiguousarray(ce[:, :, re12])
    d = np.zeros(NSYM, np.complex64)
    pd._lib().orc_ctrl_equalize(y.view(f32).ravel(), h.view(f32).ravel(), nrx, nports, NSYM,
                                float(noise) if nports == 1 else 0.0, d.view(f32))
    c = seq_float(cell_id, sf_idx)
    dr, di = (d.real * c).astype(f32), (d.imag * c).astype(f32)  # srslte_scrambling_c
    soft = np.zeros(NBITS, f32)
    with np.errstate(all="ignore"):
        for i in range(NBITS):
            zr, zi = f32(0), f32(0)
            for j in range(NSF):
                w = np.conj(W_NORMAL[nseq][j])
                xr, xi = dr[NSF * i + j], di[NSF * i + j]
                # conj(w) * d: w is +-1 or +-j, so the products are exact; then / 4, then the running sum
                if w.imag == 0:
                    tr, ti = f32(w.real) * xr, f32(w.real) * xi
                else:
                    tr, ti = f32(-w.imag) * xi, f32(w.imag) * xr
                zr = f32(zr + f32(tr / f32(NSF)))
                zi = f32(zi + f32(ti / f32(NSF)))
            # demod_bpsk_lte: -(re + im) * M_SQRT1_2, the product in double
            soft[i] = f32(np.float64(f32(-(f32(zr + zi)))) * np.float64(np.sqrt(0.5)))
        # srslte_phich_ack_decode
        best, index, dist = f32(-9999), 0, None
        for i, tab in enumerate((f32(-1), f32(1))):
            acc = f32(0)
            for b in range(NBITS):
                acc = f32(acc + f32(tab * soft[b]))
            corr = f32(acc / f32(NBITS))
            if corr > best:
                best, dist, index = corr, corr, i
    return index, dist


# ------------------------------------------------------------------ format 0 (dci.c:416-574), FDD

def _ue(cfg):
    return not getattr(cfg, "is_not_ue_ss", False)


def format0_pack(d: dict, nof_prb, nof_ports, cfg) -> np.ndarray:
    """dci_format0_pack: d has cif_present, cif, freq_hop_fl (-1 disabled), riv, mcs_idx, ndi, tpc_pusch, n_dmrs,
    cqi_request, srs_request, srs_request_present."""
    out = []
    if d.get("cif_present"):
        pd._put(out, d["cif"], 3)
    out.append(0)
    n_ul_hop = 0
    if d["freq_hop_fl"] == -1:
        out.append(0)
    else:
        out.append(1)
        if nof_prb < 50:
            n_ul_hop = 1
            out.append(d["freq_hop_fl"] & 1)
        else:
            n_ul_hop = 2
            out += [(d["freq_hop_fl"] & 2) >> 1, d["freq_hop_fl"] & 1]
    pd._put(out, d["riv"], pd.riv_nbits(nof_prb) - n_ul_hop)
    pd._put(out, d["mcs_idx"], 5)
    out.append(d["ndi"])
    pd._put(out, d["tpc_pusch"], 2)
    pd._put(out, d["n_dmrs"], 3)
    if cfg.multiple_csi_request_enabled and _ue(cfg):
        out += [d["cqi_request"], 0]
    else:
        out.append(d["cqi_request"])
    if cfg.srs_request_enabled and _ue(cfg):
        out.append(1 if (d.get("srs_request") and d.get("srs_request_present")) else 0)
    n = pd.dci_sizeof(pd.FORMAT0, nof_prb, nof_ports, cfg)
    out += [0] * (n - len(out))
    return np.array(out, np.uint8)


def format0_unpack(bits, nof_prb, cfg, ra_format_enabled=False) -> dict | None:
    """dci_format0_unpack: the fields of srsran_amd.phich.UL_FIELDS, None for a 1A payload.  Reads past the payload
    return 0 (the reference's buffer is SRSLTE_DCI_MAX_BITS long)."""
    bits = list(np.asarray(bits, np.uint8)) + [0] * 8
    d = dict(cif=0, cif_present=0, freq_hop_fl=0, riv=0, mcs_idx=0, ndi=0, tpc_pusch=0, n_dmrs=0, cqi_request=0,
             multiple_csi_request=0, multiple_csi_request_present=0, srs_request=0, srs_request_present=0, ra_type=0,
             ra_type_present=0)
    p = 0
    if cfg.cif_enabled:
        d["cif"], p = pd._take(bits, p, 3)
        d["cif_present"] = 1
    if bits[p] != 0:
        return None
    p += 1
    n_ul_hop = 0
    if bits[p] == 0:
        d["freq_hop_fl"] = -1
        p += 1
    else:
        p += 1
        n_ul_hop = 1 if nof_prb < 50 else 2
        d["freq_hop_fl"], p = pd._take(bits, p, n_ul_hop)
    d["riv"], p = pd._take(bits, p, pd.riv_nbits(nof_prb) - n_ul_hop)
    d["mcs_idx"], p = pd._take(bits, p, 5)
    d["ndi"], p = pd._take(bits, p, 1)
    d["tpc_pusch"], p = pd._take(bits, p, 2)
    d["n_dmrs"], p = pd._take(bits, p, 3)
    if cfg.multiple_csi_request_enabled and _ue(cfg):
        d["multiple_csi_request_present"] = 1
        d["multiple_csi_request"], p = pd._take(bits, p, 2)
    else:
        d["cqi_request"], p = pd._take(bits, p, 1)
    if cfg.srs_request_enabled and _ue(cfg):
        d["srs_request_present"] = 1
        d["srs_request"], p = pd._take(bits, p, 1)
    if ra_format_enabled:
        d["ra_type_present"] = 1
        d["ra_type"], p = pd._take(bits, p, 1)
    return d


# ------------------------------------------------------------------ blind search keeping the UL grants

def find_dci(llr, nof_cce, sf_idx, rnti, nof_prb, nof_ports, tm=0, cfg=None, dci_common_ss=False):
    """srslte_ue_dl_find_dl_dci followed by srslte_ue_dl_find_ul_dci (ue_dl.c:420-730) on an empty pending list:
    (dl, ul).  dl as oracle.pdcch_chain.find_dl_dci returns it; ul the pending format-0 messages in search order,
    each with L, ncce, bits and the unpacked 'dci' (format0_unpack with the UE's DCI configuration)."""
    cfg = cfg or pd.DciCfg()
    allocated, found, pending = [], [], []
    com = pd.common_locations(nof_cce)

    def overlaps(L, n):  # dci_location_is_allocated as written (see oracle.pdcch_chain.find_dl_dci)
        return any((an <= n < an + aL) or (n <= an < n + L) for (aL, an) in allocated)

    def same(a, b):  # find_dci
        return a["nof_bits"] == b["nof_bits"] and np.array_equal(a["bits"], b["bits"])

    def search(locs, formats, common):
        c = pd.DciCfg(**vars(cfg))
        if common:
            c.is_not_ue_ss = True
        out = []
        for (L, n) in locs:
            if len(found) + len(out) >= 5:
                break
            if overlaps(L, n):
                continue
            for f in formats:
                nb = pd.dci_sizeof(f, nof_prb, nof_ports, c)
                ok, bits, crc = pd.decode_candidate(llr, L, n, nb)
                if not ok or crc != rnti:
                    continue
                fmt = f
                if f in (pd.FORMAT0, pd.FORMAT1A):
                    fmt = pd.FORMAT1A if bits[3 if c.cif_enabled else 0] else pd.FORMAT0
                if dci_common_ss and (c.multiple_csi_request_enabled or c.srs_request_enabled):  # ue_dl.c:489-519
                    cc = pd.DciCfg(**vars(c))
                    cc.is_not_ue_ss = True
                    if any(cn == n for (_cl, cn) in com) and nb == pd.dci_sizeof(pd.FORMAT1A, nof_prb, nof_ports, cc):
                        fmt = pd.FORMAT1A if bits[0] else pd.FORMAT0
                msg = dict(L=L, ncce=n, format=fmt, bits=bits, nof_bits=nb)
                if fmt == pd.FORMAT0:
                    if len(pending) < 5 and not any(same(m, msg) for m in pending):
                        pending.append(msg)
                elif not any(same(m, msg) for m in out) and not any(same(m, msg) for m in pending):
                    allocated.append((L, n))
                    out.append(msg)
                    break
        return out

    if rnti in (pd.SIRNTI, pd.PRNTI) or pd.is_rar(rnti):
        found += search(com, pd.COMMON_FORMATS, True)
    else:
        found += search(pd.ue_locations(nof_cce, sf_idx, rnti), pd.UE_FORMATS[tm], False)
        if dci_common_ss:
            found += search(com, pd.COMMON_FORMATS[:1], True)
    for m in found:
        m["dci"] = pd.dci_unpack(m["bits"], m["format"], rnti, nof_prb, nof_ports, cfg)
    for m in pending:
        m["dci"] = format0_unpack(m["bits"], nof_prb, cfg)
    return found, pending
