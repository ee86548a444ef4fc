"""rclpy wrappers with the reference's node names, constructor signatures, topics and CLI flags:

    VisualLandmarkMatcher(pkl_path, log_csv)            --landmarks --out-csv [--landmarks-return --swap-flag]
                                                        [--match-policy {cross,ratio} --lowe-ratio R]
    VisualLandmarkRecorder(out_pkl, min_disp_m=2.0)     --out --min-disp
    TeachDepthMapper(out_prefix, origin_x, origin_y, width_m, height_m, res)
                                                        --out-prefix --origin-x --origin-y --width-m --height-m --res
                                                        [--depth-topic NAME --depth-k4 FX FY CX CY]
    DepthCorrelationMatcher(teach_yaml, log_csv)        --teach-map --out-csv [--depth-topic NAME --depth-k4 FX FY CX CY]
                                                        [one flag per threshold: CORRELATION_FLAGS]
    the first two, for a rectified stereo pair without a depth sensor:
                                                        [--stereo-baseline M --stereo-num-disparities N
                                                         --stereo-sgm-paths {0,4,8} --stereo-sgm-p1 N --stereo-sgm-p2 N
                                                         --stereo-cost {sad,census}
                                                         --stereo-rectify-right FILE.npz --right-topic NAME]

(reference simulation/isaac/scripts/common/visual_landmark_matcher.py:175-231,503-530,
 visual_landmark_recorder.py:154-179,375-392 and the exp-69 variant's extra flags).  They only move
data between ROS and the ROS-free cores in matcher.py / recorder.py; every feature operation runs in
the HIP library.  rclpy is imported lazily so the package imports on machines without ROS.
"""
from __future__ import annotations

import argparse
import signal
import sys

import numpy as np

from .front_end import PIXEL_FORMATS, add_front_end_flags, front_end_flags, load_mask, pixel_format_setting  # noqa: F401  (load_mask: part of this module's interface)
from .matcher import FusedLandmarkMatcher, LandmarkMatcherCore, MatcherConfig
from .recorder import LandmarkRecorderCore
from .stereo import COSTS, SGM_P1_DEFAULT, SGM_P2_DEFAULT, StereoRig

RIGHT_TOPIC = "/camera/right/image_raw"      # --right-topic: the right eye of a stereo rig (--stereo-baseline)
TICK_HZ = 2.0
CORRELATION_TICK_HZ = 1.0                    # the depth-correlation node's own rate (depth_correlation_matcher.py:51,126)
POSE_FILE = "/tmp/isaac_pose.txt"
DRIFT_FILE = "/tmp/drift_est.txt"


def img_msg_to_bgr(msg):
    buf = np.frombuffer(msg.data, dtype=np.uint8).reshape(msg.height, msg.width, 3)
    if msg.encoding == "rgb8":
        return buf[:, :, ::-1].copy()
    if msg.encoding == "bgr8":
        return buf.copy()
    raise ValueError(f"unsupported rgb encoding {msg.encoding}")


BAYER_ENCODINGS = {"bayer_rggb8": "BG", "bayer_grbg8": "GB", "bayer_bggr8": "RG", "bayer_gbrg8": "GR"}     # sensor_msgs -> OpenCV's letters


# sensor_msgs encodings of FrontEnd.pixel_format (yuv422 is UYVY, yuv422_yuy2 is YUYV; uyvy / yuyv are their newer names)
PIXEL_FORMAT_ENCODINGS = {"mono8": "mono8", "bgra8": "bgra", "rgba8": "rgba", "yuv422": "uyvy", "uyvy": "uyvy",
                          "yuv422_yuy2": "yuyv", "yuyv": "yuyv"}


def img_msg_to_frame(msg, bayer=None, pixel_format=None):
    """the colour topic's frame as the cores take it: BGR, or with bayer = "BG" / "GB" / "RG" / "GR" (FrontEnd.bayer) the
    camera's raw 8-bit mosaic, undecoded: mono8 (the driver does not name the pattern) or the bayer_* encoding of that pattern;
    or with pixel_format (FrontEnd.pixel_format) the frame of that format, undecoded: (H, W), (H, W, 4) or (H, W, 2)"""
    if pixel_format is not None:
        fmt = pixel_format_setting(pixel_format)
        if PIXEL_FORMAT_ENCODINGS.get(msg.encoding) != fmt:
            raise ValueError(f"encoding {msg.encoding} is not a frame of pixel format {fmt}")
        tail = PIXEL_FORMATS[fmt][1]
        row = msg.width * (tail[0] if tail else 1)
        step = getattr(msg, "step", 0) or row
        return np.frombuffer(msg.data, dtype=np.uint8).reshape(msg.height, step)[:, :row].reshape(msg.height, msg.width, *tail).copy()
    if bayer is None:
        return img_msg_to_bgr(msg)
    if msg.encoding != "mono8" and BAYER_ENCODINGS.get(msg.encoding) != bayer.upper():
        raise ValueError(f"encoding {msg.encoding} is not a raw 8-bit mosaic of pattern {bayer}")
    step = getattr(msg, "step", 0) or msg.width
    return np.frombuffer(msg.data, dtype=np.uint8).reshape(msg.height, step)[:, :msg.width].copy()


def img_msg_to_depth_mm(msg):
    if msg.encoding in ("16UC1", "mono16"):
        return np.frombuffer(msg.data, dtype=np.uint16).reshape(msg.height, msg.width).copy()
    if msg.encoding == "32FC1":
        mm = np.frombuffer(msg.data, dtype=np.float32).reshape(msg.height, msg.width) * 1000.0
        return np.nan_to_num(mm, nan=0.0, posinf=0.0, neginf=0.0).astype(np.uint16)
    raise ValueError(f"unexpected depth encoding {msg.encoding}")


def read_pose_file(path=POSE_FILE):
    try:
        with open(path) as f:
            parts = f.readline().split()
        return tuple(float(p) for p in parts[:7]) if len(parts) >= 7 else None
    except Exception:
        return None


def read_drift(path=DRIFT_FILE):
    try:
        with open(path) as f:
            return float(f.readline().strip())
    except Exception:
        return 0.0


def _node_base():
    from rclpy.node import Node
    return Node


def make_matcher_node(pkl_path, log_csv, return_pkl=None, swap_flag=None, global_reloc=False, fused=False, cv2=None, bayer=None,
                      mask=None, orb=None, pixel_format=None, match_policy="cross", lowe_ratio=0.8, stereo=None,
                      right_topic=RIGHT_TOPIC):
    """cv2: the cv2-shaped module the ROS-free core calls (default: the HIP shim); only the non-fused core uses it.
    bayer: FrontEnd.bayer -- the colour topic carries raw mosaics, passed through undecoded.  mask: FrontEnd.mask.
    orb: FrontEnd.orb.  pixel_format: FrontEnd.pixel_format -- the colour topic carries frames of that format, passed through
    undecoded.  match_policy, lowe_ratio: MatcherConfig's -- "cross" (the reference matcher's crossCheck) or "ratio" (knnMatch
    + Lowe test).  stereo: MatcherConfig.stereo, a StereoRig -- the right eye's frames come from right_topic (same encoding as the
    colour topic) and stand in for the depth image where none has arrived"""
    from geometry_msgs.msg import PoseWithCovarianceStamped
    from sensor_msgs.msg import Image
    Node = _node_base()

    class VisualLandmarkMatcher(Node):
        def __init__(self):
            super().__init__("visual_landmark_matcher")
            cfg = MatcherConfig(global_reloc=global_reloc, bayer=bayer, mask=mask, orb=orb, pixel_format=pixel_format,
                                match_policy=match_policy, lowe_ratio=lowe_ratio, stereo=stereo)
            if fused:
                self.core = FusedLandmarkMatcher(pkl_path, log_csv, config=cfg, return_landmarks=return_pkl,
                                                 swap_flag=swap_flag, logger=lambda m: self.get_logger().info(m),
                                                 exclusive=True)          # one node, one camera: the only work on the GPU
            else:
                self.core = LandmarkMatcherCore(pkl_path, log_csv, cv2=cv2, config=cfg, return_landmarks=return_pkl,
                                                swap_flag=swap_flag, logger=lambda m: self.get_logger().info(m))
            self.last_rgb = self.last_depth = self.last_right = None
            self.create_subscription(Image, "/camera/color/image_raw", self._rgb_cb, 10)
            self.create_subscription(Image, "/camera/depth/image_rect_raw", self._depth_cb, 10)
            if stereo is not None:
                self.create_subscription(Image, right_topic, self._right_cb, 10)
            self.anchor_pub = self.create_publisher(PoseWithCovarianceStamped, "/anchor_correction", 10)
            self.timer = self.create_timer(1.0 / TICK_HZ, self._tick)
            signal.signal(signal.SIGTERM, self._sigterm)

        def _sigterm(self, *a):
            self.core.save_augmented()
            sys.exit(0)

        def _rgb_cb(self, msg):
            try:
                self.last_rgb = img_msg_to_frame(msg, bayer, pixel_format)
            except Exception as e:
                self.get_logger().warn(f"rgb: {e}")

        def _depth_cb(self, msg):
            try:
                self.last_depth = img_msg_to_depth_mm(msg)
            except Exception as e:
                self.get_logger().warn(f"depth: {e}")

        def _right_cb(self, msg):
            try:
                self.last_right = img_msg_to_frame(msg, bayer, pixel_format)
            except Exception as e:
                self.get_logger().warn(f"right: {e}")

        def _tick(self):
            if self.last_rgb is None or (self.last_depth is None and self.last_right is None):
                return
            pose = read_pose_file()
            if pose is None:
                return
            kw = {} if stereo is None else {"right": self.last_right}
            if fused:
                o = self.core.tick(self.last_rgb, pose, depth_mm=self.last_depth, drift_est=read_drift(), **kw)
            else:
                o = self.core.tick(self.last_rgb, self.last_depth, pose, drift_est=read_drift(), **kw)
            if o is None or not o.published:
                return
            msg = PoseWithCovarianceStamped()
            msg.header.frame_id = "map"
            msg.header.stamp = self.get_clock().now().to_msg()
            p, q = msg.pose.pose.position, msg.pose.pose.orientation
            p.x, p.y, p.z = o.anchor_pose[0], o.anchor_pose[1], o.anchor_pose[2]
            q.x, q.y, q.z, q.w = o.anchor_pose[3], o.anchor_pose[4], o.anchor_pose[5], o.anchor_pose[6]
            msg.pose.covariance = o.covariance
            self.anchor_pub.publish(msg)

    return VisualLandmarkMatcher()


def make_recorder_node(out_pkl, min_disp_m=2.0, cv2=None, bayer=None, mask=None, orb=None, pixel_format=None, stereo=None,
                       right_topic=RIGHT_TOPIC):
    """stereo: a StereoRig -- the recorder takes the right eye's frames from right_topic in the depth image's place"""
    from sensor_msgs.msg import Image
    Node = _node_base()

    class VisualLandmarkRecorder(Node):
        def __init__(self):
            super().__init__("visual_landmark_recorder")
            self.core = LandmarkRecorderCore(out_pkl, min_disp_m, cv2=cv2, bayer=bayer, mask=mask, orb=orb, pixel_format=pixel_format,
                                             **({} if stereo is None else {"stereo": stereo}))
            self.last_rgb = self.last_depth = self.last_right = None
            self.last_rgb_ts = 0.0
            self.create_subscription(Image, "/camera/color/image_raw", self._rgb_cb, 10)
            self.create_subscription(Image, "/camera/depth/image_rect_raw", self._depth_cb, 10)
            if stereo is not None:
                self.create_subscription(Image, right_topic, self._right_cb, 10)
            self.timer = self.create_timer(0.2, self._tick)
            signal.signal(signal.SIGTERM, self._save_and_exit)
            signal.signal(signal.SIGINT, self._save_and_exit)

        def _rgb_cb(self, msg):
            try:
                self.last_rgb = img_msg_to_frame(msg, bayer, pixel_format)
                self.last_rgb_ts = msg.header.stamp.sec + msg.header.stamp.nanosec * 1e-9
            except Exception as e:
                self.get_logger().warn(f"rgb cb: {e}")

        def _depth_cb(self, msg):
            try:
                self.last_depth = img_msg_to_depth_mm(msg)
            except Exception as e:
                self.get_logger().warn(f"depth cb: {e}")

        def _right_cb(self, msg):
            try:
                self.last_right = img_msg_to_frame(msg, bayer, pixel_format)
            except Exception as e:
                self.get_logger().warn(f"right cb: {e}")

        def _tick(self):
            if stereo is None:
                self.core.tick(self.last_rgb, self.last_depth, read_pose_file(), self.last_rgb_ts)
            else:
                self.core.tick(self.last_rgb, self.last_depth, read_pose_file(), self.last_rgb_ts, right=self.last_right)

        def _save_and_exit(self, *a):
            self.core.save()
            sys.exit(0)

    return VisualLandmarkRecorder()


def pc2_msg_to_points(msg):
    """(n, 3) float32 x y z of a PointCloud2 with float32 fields, in the message's frame; an empty or field-less message gives
    (0, 3), like the reference mapper's _parse_pc2 (D:40-61).  Non-finite rows stay: the library drops them."""
    offsets = {f.name: f.offset for f in msg.fields}
    n = msg.width * msg.height
    if msg.point_step == 0 or n == 0 or "x" not in offsets:
        return np.zeros((0, 3), np.float32)
    rows = np.frombuffer(msg.data, dtype=np.uint8)[: n * msg.point_step].reshape(n, msg.point_step)
    cols = [rows[:, offsets[k]:offsets[k] + 4].copy().view("<f4")[:, 0] for k in ("x", "y", "z")]
    return np.stack(cols, axis=-1).astype(np.float32)


def img_msg_to_depth(msg):
    """the depth topic's image as the occupancy map takes it: float32 metres or uint16 millimetres, undecoded"""
    if msg.encoding in ("16UC1", "mono16"):
        return np.frombuffer(msg.data, dtype=np.uint16).reshape(msg.height, msg.width).copy()
    if msg.encoding == "32FC1":
        return np.frombuffer(msg.data, dtype=np.float32).reshape(msg.height, msg.width).copy()
    raise ValueError(f"unexpected depth encoding {msg.encoding}")


def make_depth_mapper_node(out_prefix, origin_x=-110.0, origin_y=-50.0, width_m=200.0, height_m=60.0, res=0.1, depth_topic=None,
                           K4=None, engine=None):
    """The reference's TeachDepthMapper(out_prefix, origin_x, origin_y, width_m, height_m, res) (teach_run_depth_mapper.py:83-111)
    over mapper.OccupancyMapperCore: /depth_points clouds, or with depth_topic that depth image itself (camera K4 = fx, fy, cx,
    cy; default the reference camera's), ray-traced on the device into the map frame of the message's frame_id.  engine: the
    Engine that holds the grid (default: a new one)."""
    import rclpy
    import rclpy.time
    import tf2_ros
    from sensor_msgs.msg import Image, PointCloud2
    from .engine import K4_DEFAULT, Engine
    from .mapper import OccupancyMapperCore, tf_to_matrix
    Node = _node_base()

    class TeachDepthMapper(Node):
        def __init__(self):
            super().__init__("teach_depth_mapper")
            self.core = OccupancyMapperCore(engine if engine is not None else Engine(), origin_x, origin_y, width_m, height_m, res,
                                            out_prefix=out_prefix)
            self.K4 = np.asarray(K4_DEFAULT if K4 is None else K4, np.float64)
            self.tf_buf = tf2_ros.Buffer()
            self.tf_listener = tf2_ros.TransformListener(self.tf_buf, self)
            self.frames_skipped_tf = 0
            if depth_topic is None:
                self.create_subscription(PointCloud2, "/depth_points", self.cb, 10)
            else:
                self.create_subscription(Image, depth_topic, self.depth_cb, 10)
            self.get_logger().info(f"Mapper grid {self.core.W}x{self.core.H} @ {res}m origin=({origin_x},{origin_y})")
            signal.signal(signal.SIGTERM, self._save_and_exit)
            signal.signal(signal.SIGINT, self._save_and_exit)
            signal.signal(signal.SIGUSR1, self._save_partial)
            self.log_timer = self.create_timer(10.0, self.log_progress)
            self.periodic_save_timer = self.create_timer(60.0, self._save_partial)

        def log_progress(self):
            c = self.core.counters()
            self.get_logger().info(f"frames: integrated={c['frames_integrated']} skipped_tf={self.frames_skipped_tf} "
                                   f"skipped_empty={c['frames_skipped_empty']} pts_total={c['total_points_integrated']}")

        def _transform(self, msg):
            """map <- the message's frame as a 3 x 4 matrix, or None (counted) when tf has none"""
            try:
                tf = self.tf_buf.lookup_transform("map", msg.header.frame_id, rclpy.time.Time()).transform
            except Exception:
                self.frames_skipped_tf += 1
                return None
            t, q = tf.translation, tf.rotation
            return tf_to_matrix((t.x, t.y, t.z), (q.x, q.y, q.z, q.w))

        def cb(self, msg):
            T = self._transform(msg)
            if T is not None:
                self.core.integrate_cloud(pc2_msg_to_points(msg), T)

        def depth_cb(self, msg):
            T = self._transform(msg)
            if T is None:
                return
            try:
                self.core.integrate_depth(img_msg_to_depth(msg), self.K4, T)
            except ValueError as e:
                self.get_logger().warn(f"depth: {e}")

        def _save_and_exit(self, *a):
            self.get_logger().warn(f"Saving map to {out_prefix}.pgm/.yaml and exiting")
            self.core.save()
            rclpy.shutdown()
            sys.exit(0)

        def _save_partial(self, *a):
            self.get_logger().info(f"[PARTIAL] saving intermediate to {out_prefix}.pgm/.yaml")
            self.core.save()

    return TeachDepthMapper()


def make_depth_correlation_node(teach_yaml, log_csv, depth_topic=None, K4=None, engine=None, **thresholds):
    """The reference's DepthCorrelationMatcher(teach_yaml, log_csv) (depth_correlation_matcher.py:111-285) over
    depth_anchor.DepthCorrelationCore: the last /depth_points cloud, or with depth_topic that depth image itself (camera K4 =
    fx, fy, cx, cy; default the reference camera's), correlated once a second against the teach map from the pose file's pose;
    an anchor goes out on /anchor_correction, beside the matcher node's.  thresholds: DepthCorrelationCore's keywords.
    engine: the Engine that holds the map (default: a new one)."""
    import time
    from geometry_msgs.msg import PoseWithCovarianceStamped
    from sensor_msgs.msg import Image, PointCloud2
    from .depth_anchor import DepthCorrelationCore
    from .engine import K4_DEFAULT, Engine
    Node = _node_base()

    class DepthCorrelationMatcher(Node):
        def __init__(self):
            super().__init__("depth_correlation_matcher")
            self.core = DepthCorrelationCore(engine if engine is not None else Engine(), teach_yaml=teach_yaml, out_csv=log_csv, **thresholds)
            self.K4 = np.asarray(K4_DEFAULT if K4 is None else K4, np.float64)
            self.last_depth = None
            if depth_topic is None:
                self.create_subscription(PointCloud2, "/depth_points", self._depth_cb, 10)
            else:
                self.create_subscription(Image, depth_topic, self._depth_cb, 10)
            self.anchor_pub = self.create_publisher(PoseWithCovarianceStamped, "/anchor_correction", 10)
            self.timer = self.create_timer(1.0 / CORRELATION_TICK_HZ, self._tick)

        def _depth_cb(self, msg):
            self.last_depth = msg

        def _tick(self):
            if self.last_depth is None:
                return
            pose = read_pose_file()
            if pose is None:
                return
            try:
                if depth_topic is None:
                    o = self.core.tick_cloud(pc2_msg_to_points(self.last_depth), pose, time.time())
                else:
                    o = self.core.tick_depth(img_msg_to_depth(self.last_depth), self.K4, pose, time.time())
            except ValueError as e:
                self.get_logger().warn(f"depth: {e}")
                return
            if o.message is None:
                return
            msg = PoseWithCovarianceStamped()
            msg.header.frame_id = o.message["frame_id"]
            msg.header.stamp = self.get_clock().now().to_msg()
            p, q = msg.pose.pose.position, msg.pose.pose.orientation
            p.x, p.y, p.z = o.message["position"]
            q.x, q.y, q.z, q.w = o.message["orientation"]
            msg.pose.covariance = o.message["covariance"]
            self.anchor_pub.publish(msg)

    return DepthCorrelationMatcher()


def _chain_args(args):
    """the trailing (cv2, bayer, mask, orb, pixel_format) of the node factories; cv2 None = the default shim; only as far as
    the last one that is not its default, nothing when all are defaults"""
    tail = [None, *front_end_flags(args), pixel_format_setting(getattr(args, "pixel_format", None))]
    while tail and tail[-1] is None:
        tail.pop()
    return tuple(tail)


class _FollowsCost(int):
    """the value of --stereo-sgm-p1 / -p2 while the flag is not given: it reads as the SAD default and tells _stereo_kwargs to
    leave the penalty to the rig, which takes the default of its cost"""


def add_stereo_flags(ap):
    """--stereo-baseline, --stereo-num-disparities, --stereo-rectify-right, --stereo-sgm-*, --stereo-cost, --right-topic: a StereoRig beside the
    front end"""
    ap.add_argument("--stereo-baseline", type=float, default=None, metavar="M",
                    help="baseline of a rectified stereo pair in metres: the right eye's frames stand in for the depth image")
    ap.add_argument("--stereo-num-disparities", type=int, default=128, metavar="N", help="searched disparities, 8..256 (default 128)")
    ap.add_argument("--stereo-rectify-right", default=None, metavar="FILE.npz",
                    help="the right eye's rectification maps: an .npz file holding map1 and map2 as cv2.remap takes them")
    ap.add_argument("--stereo-sgm-paths", type=int, default=0, choices=(0, 4, 8), metavar="{0,4,8}",
                    help="semi-global aggregation of the dense stereo pass along 4 or 8 directions (default 0: off)")
    ap.add_argument("--stereo-sgm-p1", type=int, default=_FollowsCost(SGM_P1_DEFAULT), metavar="N",
                    help=f"its penalty of a disparity step of one (default {SGM_P1_DEFAULT}; 121 with --stereo-cost census)")
    ap.add_argument("--stereo-sgm-p2", type=int, default=_FollowsCost(SGM_P2_DEFAULT), metavar="N",
                    help=f"its penalty of a larger step, p1..8191 (default {SGM_P2_DEFAULT}; 484 with --stereo-cost census)")
    ap.add_argument("--stereo-cost", default="sad", choices=COSTS,
                    help="data term of the stereo matchers: sad, or census for eyes with their own exposure and gain (default sad)")
    ap.add_argument("--right-topic", default=RIGHT_TOPIC, metavar="NAME", help="topic of the right eye's frames")


def _stereo_kwargs(args):
    """the stereo keywords of the node factories: nothing without --stereo-baseline (a bad value: ValueError)"""
    if args.stereo_baseline is None:
        return {}
    maps = None
    if args.stereo_rectify_right is not None:
        with np.load(args.stereo_rectify_right, allow_pickle=False) as z:
            maps = (z["map1"], z["map2"])
    p1, p2 = (None if isinstance(v, _FollowsCost) else v for v in (args.stereo_sgm_p1, args.stereo_sgm_p2))
    return dict(stereo=StereoRig(args.stereo_baseline, num_disparities=args.stereo_num_disparities, rectify_right=maps,
                                 sgm_paths=args.stereo_sgm_paths, sgm_p1=p1, sgm_p2=p2, cost=args.stereo_cost),
                right_topic=args.right_topic)


def _match_args(args, raw):
    """the (match_policy, lowe_ratio) of make_matcher_node behind its chain arguments `raw`, those padded to their full
    length; nothing when both are defaults"""
    policy, ratio = MatcherConfig(match_policy=args.match_policy, lowe_ratio=args.lowe_ratio).match
    if (policy, ratio) == ("cross", 0.8):
        return raw
    return (*raw, *([None] * (5 - len(raw))), policy, ratio)


def _spin(make_node, save, log_result=False):
    """one node's rclpy session: spin until interrupted, then call the core's `save` method and shut down; log_result: what
    that method returns is the node's last log line"""
    import rclpy
    rclpy.init()
    node = make_node()
    try:
        rclpy.spin(node)
    except KeyboardInterrupt:
        pass
    finally:
        out = getattr(node.core, save)()
        if log_result:
            node.get_logger().info(out)
        node.destroy_node()
        try:
            rclpy.shutdown()
        except Exception:
            pass


def matcher_main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", required=True)
    ap.add_argument("--out-csv", required=True)
    ap.add_argument("--landmarks-return", default=None)
    ap.add_argument("--swap-flag", default="/tmp/matcher_swap_return.txt")
    ap.add_argument("--global-reloc", action="store_true")
    ap.add_argument("--fused", action="store_true", help="run the whole tick in one device call")
    ap.add_argument("--match-policy", choices=("cross", "ratio"), default="cross",
                    help="cross: mutual nearest neighbours (the reference matcher); ratio: knnMatch k=2 + Lowe test")
    ap.add_argument("--lowe-ratio", type=float, default=0.8, help="ratio of the Lowe test, in (0, 1]; read under --match-policy ratio")
    add_front_end_flags(ap)
    add_stereo_flags(ap)
    args = ap.parse_args(argv)
    try:
        raw = _match_args(args, _chain_args(args))
        kw = _stereo_kwargs(args)
    except ValueError as e:
        ap.error(str(e))
    _spin(lambda: make_matcher_node(args.landmarks, args.out_csv, args.landmarks_return, args.swap_flag, args.global_reloc, args.fused, *raw, **kw),
          "save_augmented")


def recorder_main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--min-disp", type=float, default=2.0)
    add_front_end_flags(ap)
    add_stereo_flags(ap)
    args = ap.parse_args(argv)
    raw = _chain_args(args)
    try:
        kw = _stereo_kwargs(args)
    except ValueError as e:
        ap.error(str(e))
    _spin(lambda: make_recorder_node(args.out, args.min_disp, *raw, **kw), "save")


def mapper_main(argv=None):
    """the reference mapper's flags and defaults (teach_run_depth_mapper.py:242-250), plus --depth-topic / --depth-k4"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-prefix", required=True)
    ap.add_argument("--origin-x", type=float, default=-110.0)
    ap.add_argument("--origin-y", type=float, default=-50.0)
    ap.add_argument("--width-m", type=float, default=200.0)
    ap.add_argument("--height-m", type=float, default=60.0)
    ap.add_argument("--res", type=float, default=0.1)
    ap.add_argument("--depth-topic", default=None, metavar="NAME",
                    help="take this depth image topic instead of the /depth_points cloud")
    ap.add_argument("--depth-k4", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"), help="camera of --depth-topic")
    args = ap.parse_args(argv)
    tail = () if args.depth_topic is None and args.depth_k4 is None else (args.depth_topic, args.depth_k4)
    _spin(lambda: make_depth_mapper_node(args.out_prefix, args.origin_x, args.origin_y, args.width_m, args.height_m, args.res, *tail), "save")


# the thresholds of depth_correlation_main: flag, DepthCorrelationCore keyword, type, the reference's value
CORRELATION_FLAGS = (("--dilate", "dilate", int, 1), ("--window-m", "window_m", float, 5.0), ("--step-m", "step_m", float, 0.2),
                     ("--min-hits", "min_hits", int, 5), ("--min-fraction", "min_fraction", float, 0.20),
                     ("--min-peak-ratio", "min_peak_ratio", float, 1.4), ("--consistency-m", "consistency_m", float, 5.0),
                     ("--z-lo", "z_lo", float, 0.2), ("--z-hi", "z_hi", float, 2.0), ("--max-range", "max_range", float, 15.0),
                     ("--min-points", "min_points", int, 100))


def depth_correlation_args(argv=None):
    """(teach_map, out_csv, tail, thresholds) of depth_correlation_main's command line: the reference matcher's two flags
    (depth_correlation_matcher.py:287-291), --depth-topic / --depth-k4 as mapper_main has them, one flag per threshold; tail and
    thresholds hold only what differs from the defaults"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--teach-map", required=True)
    ap.add_argument("--out-csv", required=True)
    ap.add_argument("--depth-topic", default=None, metavar="NAME",
                    help="take this depth image topic instead of the /depth_points cloud")
    ap.add_argument("--depth-k4", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"), help="camera of --depth-topic")
    for flag, key, ty, default in CORRELATION_FLAGS:
        ap.add_argument(flag, dest=key, type=ty, default=default, help=f"default {default}")
    args = ap.parse_args(argv)
    tail = () if args.depth_topic is None and args.depth_k4 is None else (args.depth_topic, args.depth_k4)
    thresholds = {key: getattr(args, key) for _, key, _, default in CORRELATION_FLAGS if getattr(args, key) != default}
    return args.teach_map, args.out_csv, tail, thresholds


def depth_correlation_main(argv=None):
    """on shutdown the node logs the reference's `Final: N publishes / M attempts` (depth_correlation_matcher.py:300-301)"""
    teach_map, out_csv, tail, thresholds = depth_correlation_args(argv)
    _spin(lambda: make_depth_correlation_node(teach_map, out_csv, *tail, **thresholds), "summary", log_result=True)


def make_goal_projector(waypoints, engine=None, **thresholds):
    """send_goals_hybrid.py's proactive projection (its costmap_cb, :235-262) without the planner client: a ROS-free holder whose
    costmap_cb takes an OccupancyGrid-shaped message (info.width / height / resolution / origin.position, data) and re-projects
    the waypoints from current_idx on through route.WaypointProjectorCore; projected_wps, skip_flags and the two counters are the
    core's.  thresholds: WaypointProjectorCore's keywords.  engine: the Engine that holds the costmap (default: a new one)."""
    from .route import WaypointProjectorCore
    if engine is None:
        from .engine import Engine
        engine = Engine()

    class GoalProjector:
        def __init__(self):
            self.core = WaypointProjectorCore(engine, waypoints, **thresholds)
            self.current_idx = 0

        def costmap_cb(self, msg):
            info = msg.info
            cost = np.array(msg.data, dtype=np.int8).reshape(info.height, info.width)
            return self.core.costmap_update(cost, info.origin.position.x, info.origin.position.y, info.resolution, self.current_idx)

    return GoalProjector()


def sanitize_route_main(argv=None, engine=None):
    """sanitize_route.py's flags (its main, :133-141) plus the obstacles it hard-codes as arguments: --cone X Y (repeatable) and
    --tent CX CY HX HY; prints the reference's summary lines.  engine: the Engine to run on (default: a new one)."""
    import csv
    from .route import RouteSanitizerCore
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectory", required=True, help="input CSV with gt_x, gt_y columns")
    ap.add_argument("--teach-map", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--spacing", type=float, default=4.0, help="only sanitize WPs at this spacing")
    ap.add_argument("--cone", type=float, nargs=2, action="append", default=[], metavar=("X", "Y"), help="a known cone, one cell; repeatable")
    ap.add_argument("--tent", type=float, nargs=4, default=None, metavar=("CX", "CY", "HX", "HY"), help="a known tent: centre and half extents")
    args = ap.parse_args(argv)
    if engine is None:
        from .engine import Engine
        engine = Engine()
    core = RouteSanitizerCore(engine, teach_yaml=args.teach_map, cones=[tuple(c) for c in args.cone], tent=args.tent)
    with open(args.trajectory) as f:
        pts = [(float(row["gt_x"]), float(row["gt_y"])) for row in csv.DictReader(f)]
    wps = core.subsample(pts, args.spacing)
    print(f"Loaded {len(wps)} WPs at {args.spacing}m spacing")
    rows, counts = core.sanitize(wps)
    core.write_csv(args.output, rows)
    print(f"\nWrote {len(rows)} rows to {args.output}")
    print(f"  safe unchanged:  {counts['unchanged']}")
    print(f"  shifted:         {counts['shifted']}")
    print(f"  skipped (unsafe):{counts['skipped']}")
    return counts
