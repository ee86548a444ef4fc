"""What tests/test_gpu_scan.py expects of the scan half of a tick, restated in float64 NumPy from csrc/reloc_internal.h and
csrc/reloc_db.hip (the counting itself is the oracle's): the heading mask of a whole-database scan -- record_heading of the
database index, cur_heading_q of the frame's base_link quaternion, heading_ok -- in the kernels' operation order, the masked
expectation of a scan, its ranking as the rows of reloc_tick_scan_dev / reloc_shard_scan_batch_dev carry it, and the launch
arithmetic that decides whether a scan draws tickets.  Imported like match_policy_ref."""
import numpy as np

B2C_ROW0 = (0.0, -1.0, 0.0)              # first row of the default base_link -> camera rotation (CameraModel::b2c_R)
MAX_REC_ROWS = 4096                      # csrc/reloc_internal.h
SQ_MAX_ROWS = 1024                       # the lane-per-row kernel's largest record (csrc/reloc_hamming.h)
BATCH_MAX = 8                            # RELOC_BATCH_MAX
WG_PER_CU = 4                            # resident scan workgroups per CU (CountPlan::init)


def record_heading(poses, b=B2C_ROW0):
    """(cos, sin) of the heading of base_link +X in the world per stored CAMERA pose (x y z qx qy qz qw): record_heading of
    csrc/reloc_db.hip, what k_db_index files in the database index"""
    p = np.asarray(poses, np.float64).reshape(-1, 7)
    qx, qy, qz, qw = p[:, 3], p[:, 4], p[:, 5], p[:, 6]
    r00, r01, r02 = 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)
    r10, r11, r12 = 2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)
    fx = r00 * b[0] + r01 * b[1] + r02 * b[2]
    fy = r10 * b[0] + r11 * b[1] + r12 * b[2]
    fn = np.sqrt(fx * fx + fy * fy)
    ok = fn > 0
    safe = np.where(ok, fn, 1.0)
    return np.where(ok, fx / safe, 1.0), np.where(ok, fy / safe, 0.0)


def cur_heading_q(q):
    """(cos, sin) of the robot's heading from its base_link quaternion (x, y, z, w): cur_heading_q of csrc/reloc_internal.h"""
    qx, qy, qz, qw = (float(v) for v in q)
    r00 = 1 - 2 * (qy * qy + qz * qz)
    r10 = 2 * (qx * qy + qz * qw)
    n = np.sqrt(r00 * r00 + r10 * r10)
    return (r00 / n, r10 / n) if n > 0 else (1.0, 0.0)


def cos_tol(heading_tol_deg):
    """heading_cos_tol_host of csrc/reloc_tick.hip"""
    return float(np.cos(heading_tol_deg * 3.14159265358979323846 / 180.0))


def heading_cos(poses, base_pose):
    """per record cos(teach heading - current heading), the left side of heading_ok"""
    ch, sh = record_heading(poses)
    cc, sc = cur_heading_q(base_pose[3:7])
    return ch * cc + sh * sc


def heading_ok(poses, base_pose, heading_tol_deg):
    """(compatible per record, the smallest |cos(delta) - cos_tol| over the records): the second is the margin by which the
    float64 restatement (about 1e-15 of rounding) cannot flip a record"""
    c, t = heading_cos(poses, base_pose), cos_tol(heading_tol_deg)
    return c > t, float(np.abs(c - t).min())


def masked(counts, compatible=None):
    """the counts a scan leaves: 0 on heading-incompatible records (ScanMask); compatible None: no mask"""
    counts = np.asarray(counts, np.int32)
    return counts.copy() if compatible is None else np.where(compatible, counts, 0).astype(np.int32)


def ratio_gate(counts, rows, min_matches):
    """the record-length gate of the ratio scan (db_ratio_body<true>): a record of fewer than min_matches rows counts 0"""
    return np.where(np.asarray(rows) >= min_matches, counts, 0).astype(np.int32)


def ranking(oracle, expected, min_matches, k, id_base=0):
    """(k ids + id_base, -1 padded; k counts, 0 padded): the top-k of (count, id) among the records of at least min_matches, as
    k_topk_counts writes it"""
    top = oracle.topk_records(expected, min_matches, k)
    ids = np.full(k, -1, np.int32)
    cnt = np.zeros(k, np.int32)
    ids[:len(top)] = top + id_base
    cnt[:len(top)] = np.asarray(expected)[top]
    return ids, cnt


def single_scan_draws_tickets(n_records, num_cu):
    """launch_db_count with the 8-column kernel: records are drawn from the ticket counters when they outnumber one resident
    generation of workgroups (at most WG_PER_CU per CU)"""
    return n_records > WG_PER_CU * num_cu


def batch_scan_draws_tickets(n_records, num_cu, n_frames):
    """launch_db_scan_batch: per frame at most ceil(WG_PER_CU * num_cu / n) budgeted workgroups and one sweeper; tickets are
    drawn when the records outnumber them"""
    return n_records > -(-WG_PER_CU * num_cu // n_frames) + 1
