"""The cases of test_annotate_options_cpu.py (host only): the option sets, the bad combinations and the command lines, and behind the
line "recorded" what each of them did -- literals, recorded as that test's docstring says."""
TRACK = (30, 8, 0)
MOTION = dict(track=TRACK, track_motion=8)
REDACT = (("car",), "pixelate", 16, 0)
COUNT = (((0, 0, 8, 8),), "all", None)
ZONE = ((((0, 0), (8, 0), (8, 8)),), "all", None, None)
REGION = ((((0, 0), (4, 0), (4, 4)),), None, None, None, None)

# one set per option, each with what it needs (an output: the file's name; "tracks_out": an open text file), and one of all that combine
OPTIONS = {
    "plain": {},
    "redact": dict(redact=REDACT),
    "draw": dict(draw=False),
    "track": dict(track=TRACK, tracks_out="tracks.txt"),
    "track_motion": MOTION,
    "track_lookback": dict(track=TRACK, track_lookback=2),
    "track_lookback_auto": dict(track=TRACK, track_lookback=0),
    "detect_every": dict(MOTION, detect_every=2),
    "track_backtrack": dict(MOTION, detect_every=2, track_backtrack=2),
    "track_scene_cut": dict(MOTION, track_scene_cut=40),
    "track_trails": dict(track=TRACK, track_trails=(16, 3)),
    "heatmap": dict(heatmap=("all", None, None), heatmap_out="heat.png"),
    "count": dict(track=TRACK, count=COUNT, counts_out="counts.csv"),
    "zone": dict(track=TRACK, zone=ZONE, zones_out="zones.csv"),
    "remove": dict(remove=(("car",), None, None, None), plate_out="plate.png"),
    "track_reid": dict(track=TRACK, track_reid=(25, None), reid_out="reid.csv"),
    "post": dict(post="soft_linear"),
    "out_size": dict(out_size=("scale", 2)),
    "redact_shape": dict(redact=REDACT, redact_shape=("ellipse", 4)),
    "redact_shape_box": dict(redact=REDACT, redact_shape=("box", 0)),
    "det_threshold": dict(det_threshold=0.5),
    "track_low": dict(track=TRACK, det_threshold=0.5, track_low=0.25),
    "redact_region": dict(redact_region=REGION),
    "redact_moving": dict(redact_moving=True, moving_out="moving.csv"),
    "redact_moving_remove": dict(redact_moving={"tol": 30}, remove=("all", 4, None, None), redact_region=REGION, plate_out="plate.png"),
    "everything": dict(redact=REDACT, draw=True, track=TRACK, tracks_out="tracks.txt", track_motion=8, detect_every=2, track_scene_cut=40,
                       track_trails=(16, 3), heatmap=("all", None, None), heatmap_out="heat.png", count=COUNT, counts_out="counts.csv",
                       zone=ZONE, zones_out="zones.csv", remove=(("car",), None, None, None), plate_out="plate.png", track_reid=(25, None),
                       reid_out="reid.csv", post="soft_linear", out_size=("scale", 2), redact_shape=("ellipse", 4), det_threshold=0.5,
                       track_low=0.25, redact_region=REGION, redact_moving=True, moving_out="moving.csv"),
}

# bad combinations: every "needs X" and "not together with Y" of the entry points, and two with two violations at once
REFUSALS = {
    "motion_needs_track": dict(track_motion=8),
    "lookback_needs_track": dict(track_lookback=2),
    "every_needs_motion": dict(track=TRACK, detect_every=2),
    "every_with_lookback": dict(MOTION, detect_every=2, track_lookback=2),
    "backtrack_needs_every": dict(MOTION, track_backtrack=2),
    "backtrack_with_lookback": dict(MOTION, track_backtrack=2, track_lookback=2),
    "cut_needs_motion": dict(track=TRACK, track_scene_cut=40),
    "cut_with_lookback": dict(MOTION, track_scene_cut=40, track_lookback=2),
    "cut_with_backtrack": dict(MOTION, detect_every=2, track_backtrack=2, track_scene_cut=40),
    "trails_need_track": dict(track_trails=(16, 3)),
    "trails_with_no_draw": dict(track=TRACK, track_trails=(16, 3), draw=False),
    "heatmap_out_needs_heatmap": dict(heatmap_out="heat.png"),
    "heatmap_out_not_png": dict(heatmap=("all", None, None), heatmap_out="heat.csv"),
    "count_needs_track": dict(count=COUNT),
    "counts_out_needs_count": dict(counts_out="counts.csv"),
    "zone_needs_track": dict(zone=ZONE),
    "zones_out_needs_zone": dict(zones_out="zones.csv"),
    "remove_unknown_class": dict(remove=(("cat",), None, None, None)),
    "plate_out_needs_remove": dict(plate_out="plate.png"),
    "reid_needs_track": dict(track_reid=(25, None)),
    "reid_out_needs_reid": dict(track=TRACK, reid_out="reid.csv"),
    "reid_with_lookback": dict(track=TRACK, track_reid=(25, None), track_lookback=2),
    "reid_with_backtrack": dict(MOTION, detect_every=2, track_backtrack=2, track_reid=(25, None)),
    "shape_needs_redact": dict(redact_shape=("ellipse", 4)),
    "low_needs_track": dict(det_threshold=0.5, track_low=0.25),
    "low_not_under_threshold": dict(track=TRACK, det_threshold=0.25, track_low=0.5),
    "moving_out_needs_moving": dict(moving_out="moving.csv"),
    "moving_plate_differs": dict(redact_moving={"settle": 3}, remove=("all", 4, None, None)),
    "lookback_on_one_frame": dict(track=TRACK, track_lookback=2),
    "every_on_one_frame": dict(MOTION, detect_every=2),
    "backtrack_on_one_frame": dict(MOTION, detect_every=2, track_backtrack=2),
    "two_need_track": dict(track_motion=8, count=COUNT, zone=ZONE, track_reid=(25, None)),
    "two_outputs_and_a_shape": dict(counts_out="counts.csv", zones_out="zones.csv", redact_shape=("ellipse", 4), post="no such mode"),
}

# command lines behind ``s3.h5 s4.h5 <tmp>/in`` (VOC classes)
_ALL = ["--redact", "car", "--redact_mode", "blur", "--redact_size", "5", "--redact_margin", "2", "--redact_shape", "ellipse", "--redact_feather", "4",
        "--track", "--track_iou", "40", "--track_hold", "4", "--track_grow", "1", "--tracks_out", "<tmp>/tracks.txt", "--track_motion",
        "--detect_every", "2", "--track_scene_cut", "--track_reid", "--reid_keep", "100", "--reid_out", "<tmp>/reid.csv", "--track_trails",
        "--trail_width", "5", "--heatmap", "all", "--heatmap_alpha", "100", "--heatmap_decay", "2", "--heatmap_out", "<tmp>/heat.png",
        "--remove", "person", "--remove_settle", "4", "--remove_tol", "5", "--remove_margin", "3", "--plate_out", "<tmp>/plate.png",
        "--count_line", "0,0,8,8", "--count_classes", "car", "--count_width", "2", "--counts_out", "<tmp>/counts.csv",
        "--zone", "0,0,8,0,8,8", "--zone_classes", "car", "--zone_width", "2", "--zone_anchor", "bottom", "--zones_out", "<tmp>/zones.csv",
        "--det_threshold", "0.5", "--track_low", "0.25", "--redact_region", "0,0,4,0,4,4", "--region_mode", "blur", "--region_size", "3",
        "--region_feather", "2", "--redact_moving", "--moving_tol", "30", "--moving_min", "4", "--moving_hold", "2", "--moving_grow", "3",
        "--moving_feather", "1", "--moving_unknown", "hide", "--moving_except", "car", "--moving_mode", "fill", "--moving_out",
        "<tmp>/moving.csv", "--nms", "soft_linear", "--out_scale", "2"]
COMMAND_LINES = {
    "bare": ["--out_dir", "<tmp>/out"],
    "every_option": ["--out_dir", "<tmp>/out"] + _ALL,
    "every_option_to_a_video": ["--out_video", "<tmp>/out.y4m"] + _ALL,
    "no_draw_and_lookback": ["--out_dir", "<tmp>/out", "--no_draw", "--track", "--track_lookback"],
    "backtrack": ["--out_dir", "<tmp>/out", "--track", "--track_motion", "4", "--detect_every", "3", "--track_backtrack"],
}

# --------------------------------------------------------------------------------------------------------------------------- recorded
LISTS = {'plain': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
           'keywords': [('annotate', True)],
           'thresholds': [0.0],
           'said': 'processing <in>/f00.png\n'
                   'num rois: 0\n'
                   'processing <in>/f01.png\n'
                   'num rois: 0\n'
                   'processing <in>/f02.png\n'
                   'num rois: 0\n'
                   'processing <in>/f03.png\n'
                   'num rois: 0\n'
                   'processing <in>/f04.png\n'
                   'num rois: 0\n'
                   'processing <in>/f05.png\n'
                   'num rois: 0\n'
                   'processing <in>/f06.png\n'
                   'num rois: 0\n',
           'heatmaps': [],
           'files': {},
           'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                      ['frame_000000.png',
                       'frame_000001.png',
                       'frame_000002.png',
                       'frame_000003.png',
                       'frame_000004.png',
                       'frame_000005.png',
                       'frame_000006.png'])},
 'redact': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
            'keywords': [('annotate', True), ('draw', True), ('redact', (('car',), 'pixelate', 16, 0))],
            'thresholds': [0.0],
            'said': 'processing <in>/f00.png\n'
                    'num rois: 0\n'
                    'processing <in>/f01.png\n'
                    'num rois: 0\n'
                    'processing <in>/f02.png\n'
                    'num rois: 0\n'
                    'processing <in>/f03.png\n'
                    'num rois: 0\n'
                    'processing <in>/f04.png\n'
                    'num rois: 0\n'
                    'processing <in>/f05.png\n'
                    'num rois: 0\n'
                    'processing <in>/f06.png\n'
                    'num rois: 0\n',
            'heatmaps': [],
            'files': {},
            'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                       ['frame_000000.png',
                        'frame_000001.png',
                        'frame_000002.png',
                        'frame_000003.png',
                        'frame_000004.png',
                        'frame_000005.png',
                        'frame_000006.png'])},
 'draw': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
          'keywords': [('annotate', True), ('draw', False)],
          'thresholds': [0.0],
          'said': 'processing <in>/f00.png\n'
                  'num rois: 0\n'
                  'processing <in>/f01.png\n'
                  'num rois: 0\n'
                  'processing <in>/f02.png\n'
                  'num rois: 0\n'
                  'processing <in>/f03.png\n'
                  'num rois: 0\n'
                  'processing <in>/f04.png\n'
                  'num rois: 0\n'
                  'processing <in>/f05.png\n'
                  'num rois: 0\n'
                  'processing <in>/f06.png\n'
                  'num rois: 0\n',
          'heatmaps': [],
          'files': {},
          'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                     ['frame_000000.png',
                      'frame_000001.png',
                      'frame_000002.png',
                      'frame_000003.png',
                      'frame_000004.png',
                      'frame_000005.png',
                      'frame_000006.png'])},
 'track': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
           'keywords': [('annotate', True), ('track', (30, 8, 0))],
           'thresholds': [0.0],
           'said': 'processing <in>/f00.png\n'
                   'num rois: 0\n'
                   'processing <in>/f01.png\n'
                   'num rois: 0\n'
                   'processing <in>/f02.png\n'
                   'num rois: 0\n'
                   'processing <in>/f03.png\n'
                   'num rois: 0\n'
                   'processing <in>/f04.png\n'
                   'num rois: 0\n'
                   'processing <in>/f05.png\n'
                   'num rois: 0\n'
                   'processing <in>/f06.png\n'
                   'num rois: 0\n',
           'heatmaps': [],
           'files': {'tracks_out': ''},
           'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                      ['frame_000000.png',
                       'frame_000001.png',
                       'frame_000002.png',
                       'frame_000003.png',
                       'frame_000004.png',
                       'frame_000005.png',
                       'frame_000006.png'])},
 'track_motion': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                  'keywords': [('annotate', True), ('track', (30, 8, 0)), ('track_motion', 8)],
                  'thresholds': [0.0],
                  'said': 'processing <in>/f00.png\n'
                          'num rois: 0\n'
                          'processing <in>/f01.png\n'
                          'num rois: 0\n'
                          'processing <in>/f02.png\n'
                          'num rois: 0\n'
                          'processing <in>/f03.png\n'
                          'num rois: 0\n'
                          'processing <in>/f04.png\n'
                          'num rois: 0\n'
                          'processing <in>/f05.png\n'
                          'num rois: 0\n'
                          'processing <in>/f06.png\n'
                          'num rois: 0\n',
                  'heatmaps': [],
                  'files': {},
                  'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                             ['frame_000000.png',
                              'frame_000001.png',
                              'frame_000002.png',
                              'frame_000003.png',
                              'frame_000004.png',
                              'frame_000005.png',
                              'frame_000006.png'])},
 'track_lookback': {'passes': [(4, 4, 4), (1, 1, 4), (0, 0, 4), (2, 2, 4), (0, 0, 4)],
                    'keywords': [('annotate', True), ('track', (30, 8, 0)), ('track_lookback', 2)],
                    'thresholds': [0.0],
                    'said': 'processing <in>/f00.png\n'
                            'num rois: 0\n'
                            'processing <in>/f01.png\n'
                            'num rois: 0\n'
                            'processing <in>/f02.png\n'
                            'num rois: 0\n'
                            'processing <in>/f03.png\n'
                            'num rois: 0\n'
                            'processing <in>/f04.png\n'
                            'num rois: 0\n'
                            'processing <in>/f05.png\n'
                            'num rois: 0\n'
                            'processing <in>/f06.png\n'
                            'num rois: 0\n',
                    'heatmaps': [],
                    'files': {},
                    'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                               ['frame_000000.png',
                                'frame_000001.png',
                                'frame_000002.png',
                                'frame_000003.png',
                                'frame_000004.png',
                                'frame_000005.png',
                                'frame_000006.png'])},
 'track_lookback_auto': {'passes': [(4, 4, 4), (1, 1, 4), (0, 0, 4), (2, 2, 4), (0, 0, 4)],
                         'keywords': [('annotate', True), ('track', (30, 8, 0)), ('track_lookback', 4)],
                         'thresholds': [0.0],
                         'said': 'processing <in>/f00.png\n'
                                 'num rois: 0\n'
                                 'processing <in>/f01.png\n'
                                 'num rois: 0\n'
                                 'processing <in>/f02.png\n'
                                 'num rois: 0\n'
                                 'processing <in>/f03.png\n'
                                 'num rois: 0\n'
                                 'processing <in>/f04.png\n'
                                 'num rois: 0\n'
                                 'processing <in>/f05.png\n'
                                 'num rois: 0\n'
                                 'processing <in>/f06.png\n'
                                 'num rois: 0\n',
                         'heatmaps': [],
                         'files': {},
                         'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                                    ['frame_000000.png',
                                     'frame_000001.png',
                                     'frame_000002.png',
                                     'frame_000003.png',
                                     'frame_000004.png',
                                     'frame_000005.png',
                                     'frame_000006.png'])},
 'detect_every': {'passes': [(3, 5, 4), (1, 2, 1)],
                  'keywords': [('annotate', True), ('detect_every', 2), ('track', (30, 8, 0)), ('track_motion', 8)],
                  'thresholds': [0.0],
                  'said': 'processing <in>/f00.png\n'
                          'num rois: 0\n'
                          'processing <in>/f01.png\n'
                          'num rois: 0\n'
                          'processing <in>/f02.png\n'
                          'num rois: 0\n'
                          'processing <in>/f03.png\n'
                          'num rois: 0\n'
                          'processing <in>/f04.png\n'
                          'num rois: 0\n'
                          'processing <in>/f05.png\n'
                          'num rois: 0\n'
                          'processing <in>/f06.png\n'
                          'num rois: 0\n',
                  'heatmaps': [],
                  'files': {},
                  'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                             ['frame_000000.png',
                              'frame_000001.png',
                              'frame_000002.png',
                              'frame_000003.png',
                              'frame_000004.png',
                              'frame_000005.png',
                              'frame_000006.png'])},
 'track_backtrack': {'passes': [(3, 5, 4), (0, 0, 4), (1, 2, 4), (0, 0, 4)],
                     'keywords': [('annotate', True),
                                  ('detect_every', 2),
                                  ('track', (30, 8, 0)),
                                  ('track_backtrack', 2),
                                  ('track_motion', 8)],
                     'thresholds': [0.0],
                     'said': 'processing <in>/f00.png\n'
                             'num rois: 0\n'
                             'processing <in>/f01.png\n'
                             'num rois: 0\n'
                             'processing <in>/f02.png\n'
                             'num rois: 0\n'
                             'processing <in>/f03.png\n'
                             'num rois: 0\n'
                             'processing <in>/f04.png\n'
                             'num rois: 0\n'
                             'processing <in>/f05.png\n'
                             'num rois: 0\n'
                             'processing <in>/f06.png\n'
                             'num rois: 0\n',
                     'heatmaps': [],
                     'files': {},
                     'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                                ['frame_000000.png',
                                 'frame_000001.png',
                                 'frame_000002.png',
                                 'frame_000003.png',
                                 'frame_000004.png',
                                 'frame_000005.png',
                                 'frame_000006.png'])},
 'track_scene_cut': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                     'keywords': [('annotate', True), ('track', (30, 8, 0)), ('track_motion', 8), ('track_scene_cut', 40)],
                     'thresholds': [0.0],
                     'said': 'processing <in>/f00.png\n'
                             'num rois: 0\n'
                             'processing <in>/f01.png\n'
                             'num rois: 0\n'
                             'processing <in>/f02.png\n'
                             'num rois: 0\n'
                             'processing <in>/f03.png\n'
                             'num rois: 0\n'
                             'processing <in>/f04.png\n'
                             'num rois: 0\n'
                             'processing <in>/f05.png\n'
                             'num rois: 0\n'
                             'processing <in>/f06.png\n'
                             'num rois: 0\n',
                     'heatmaps': [],
                     'files': {},
                     'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                                ['frame_000000.png',
                                 'frame_000001.png',
                                 'frame_000002.png',
                                 'frame_000003.png',
                                 'frame_000004.png',
                                 'frame_000005.png',
                                 'frame_000006.png'])},
 'track_trails': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                  'keywords': [('annotate', True), ('track', (30, 8, 0)), ('track_trails', (16, 3))],
                  'thresholds': [0.0],
                  'said': 'processing <in>/f00.png\n'
                          'num rois: 0\n'
                          'processing <in>/f01.png\n'
                          'num rois: 0\n'
                          'processing <in>/f02.png\n'
                          'num rois: 0\n'
                          'processing <in>/f03.png\n'
                          'num rois: 0\n'
                          'processing <in>/f04.png\n'
                          'num rois: 0\n'
                          'processing <in>/f05.png\n'
                          'num rois: 0\n'
                          'processing <in>/f06.png\n'
                          'num rois: 0\n',
                  'heatmaps': [],
                  'files': {},
                  'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                             ['frame_000000.png',
                              'frame_000001.png',
                              'frame_000002.png',
                              'frame_000003.png',
                              'frame_000004.png',
                              'frame_000005.png',
                              'frame_000006.png'])},
 'heatmap': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
             'keywords': [('annotate', True), ('heat', ('all', 160, 0))],
             'thresholds': [0.0],
             'said': 'processing <in>/f00.png\n'
                     'num rois: 0\n'
                     'processing <in>/f01.png\n'
                     'num rois: 0\n'
                     'processing <in>/f02.png\n'
                     'num rois: 0\n'
                     'processing <in>/f03.png\n'
                     'num rois: 0\n'
                     'processing <in>/f04.png\n'
                     'num rois: 0\n'
                     'processing <in>/f05.png\n'
                     'num rois: 0\n'
                     'processing <in>/f06.png\n'
                     'num rois: 0\n',
             'heatmaps': ['heat.png'],
             'files': {},
             'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                        ['frame_000000.png',
                         'frame_000001.png',
                         'frame_000002.png',
                         'frame_000003.png',
                         'frame_000004.png',
                         'frame_000005.png',
                         'frame_000006.png'])},
 'count': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
           'keywords': [('annotate', True), ('count', (((0, 0, 8, 8),), 'all', 3)), ('track', (30, 8, 0))],
           'thresholds': [0.0],
           'said': 'processing <in>/f00.png\n'
                   'num rois: 0\n'
                   'processing <in>/f01.png\n'
                   'num rois: 0\n'
                   'processing <in>/f02.png\n'
                   'num rois: 0\n'
                   'processing <in>/f03.png\n'
                   'num rois: 0\n'
                   'processing <in>/f04.png\n'
                   'num rois: 0\n'
                   'processing <in>/f05.png\n'
                   'num rois: 0\n'
                   'processing <in>/f06.png\n'
                   'num rois: 0\n'
                   'line 0: +2 -1\n'
                   "warning: 3 crossings did not fit their frames' lists: the counts file is short by that many rows; the totals are "
                   'exact\n',
           'heatmaps': [],
           'files': {'counts.csv': 'frame,line,direction,id,cls\n'},
           'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                      ['frame_000000.png',
                       'frame_000001.png',
                       'frame_000002.png',
                       'frame_000003.png',
                       'frame_000004.png',
                       'frame_000005.png',
                       'frame_000006.png'])},
 'zone': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
          'keywords': [('annotate', True), ('track', (30, 8, 0)), ('zone', ((((0, 0), (8, 0), (8, 8)),), 'all', 3, 0))],
          'thresholds': [0.0],
          'said': 'processing <in>/f00.png\n'
                  'num rois: 0\n'
                  'processing <in>/f01.png\n'
                  'num rois: 0\n'
                  'processing <in>/f02.png\n'
                  'num rois: 0\n'
                  'processing <in>/f03.png\n'
                  'num rois: 0\n'
                  'processing <in>/f04.png\n'
                  'num rois: 0\n'
                  'processing <in>/f05.png\n'
                  'num rois: 0\n'
                  'processing <in>/f06.png\n'
                  'num rois: 0\n'
                  'zone 0: visitors 4 peak 2 stays 2 mean dwell 4.5 frames\n'
                  "warning: 1 zone events did not fit their frames' lists: the zones file is short by that many rows; the totals are "
                  'exact\n',
          'heatmaps': [],
          'files': {'zones.csv': 'frame,zone,kind,id,cls,dwell\n'},
          'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                     ['frame_000000.png',
                      'frame_000001.png',
                      'frame_000002.png',
                      'frame_000003.png',
                      'frame_000004.png',
                      'frame_000005.png',
                      'frame_000006.png'])},
 'remove': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
            'keywords': [('annotate', True), ('remove', (('car',), 8, 10, 8))],
            'thresholds': [0.0],
            'said': 'processing <in>/f00.png\n'
                    'num rois: 0\n'
                    'processing <in>/f01.png\n'
                    'num rois: 0\n'
                    'processing <in>/f02.png\n'
                    'num rois: 0\n'
                    'processing <in>/f03.png\n'
                    'num rois: 0\n'
                    'processing <in>/f04.png\n'
                    'num rois: 0\n'
                    'processing <in>/f05.png\n'
                    'num rois: 0\n'
                    'processing <in>/f06.png\n'
                    'num rois: 0\n'
                    'plate 8x6: 2 frames, 25.0 % known\n'
                    'plate 8x8: 5 frames, 75.0 % known\n',
            'heatmaps': [],
            'files': {'plate_8x6.png': None, 'plate_8x8.png': None},
            'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                       ['frame_000000.png',
                        'frame_000001.png',
                        'frame_000002.png',
                        'frame_000003.png',
                        'frame_000004.png',
                        'frame_000005.png',
                        'frame_000006.png'])},
 'track_reid': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                'keywords': [('annotate', True), ('track', (30, 8, 0)), ('track_reid', (25, 250))],
                'thresholds': [0.0],
                'said': 'processing <in>/f00.png\n'
                        'num rois: 0\n'
                        'processing <in>/f01.png\n'
                        'num rois: 0\n'
                        'processing <in>/f02.png\n'
                        'num rois: 0\n'
                        'processing <in>/f03.png\n'
                        'num rois: 0\n'
                        'processing <in>/f04.png\n'
                        'num rois: 0\n'
                        'processing <in>/f05.png\n'
                        'num rois: 0\n'
                        'processing <in>/f06.png\n'
                        'num rois: 0\n'
                        're-identified: 0\n',
                'heatmaps': [],
                'files': {'reid.csv': 'frame,id,tracker_id,cls,distance,gap\n'},
                'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                           ['frame_000000.png',
                            'frame_000001.png',
                            'frame_000002.png',
                            'frame_000003.png',
                            'frame_000004.png',
                            'frame_000005.png',
                            'frame_000006.png'])},
 'post': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
          'keywords': [('annotate', True)],
          'thresholds': [0.0],
          'said': 'processing <in>/f00.png\n'
                  'num rois: 0\n'
                  'processing <in>/f01.png\n'
                  'num rois: 0\n'
                  'processing <in>/f02.png\n'
                  'num rois: 0\n'
                  'processing <in>/f03.png\n'
                  'num rois: 0\n'
                  'processing <in>/f04.png\n'
                  'num rois: 0\n'
                  'processing <in>/f05.png\n'
                  'num rois: 0\n'
                  'processing <in>/f06.png\n'
                  'num rois: 0\n',
          'heatmaps': [],
          'files': {},
          'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                     ['frame_000000.png',
                      'frame_000001.png',
                      'frame_000002.png',
                      'frame_000003.png',
                      'frame_000004.png',
                      'frame_000005.png',
                      'frame_000006.png'])},
 'out_size': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
              'keywords': [('annotate', True), ('out_size', ('scale', 2))],
              'thresholds': [0.0],
              'said': 'processing <in>/f00.png\n'
                      'num rois: 0\n'
                      'processing <in>/f01.png\n'
                      'num rois: 0\n'
                      'processing <in>/f02.png\n'
                      'num rois: 0\n'
                      'processing <in>/f03.png\n'
                      'num rois: 0\n'
                      'processing <in>/f04.png\n'
                      'num rois: 0\n'
                      'processing <in>/f05.png\n'
                      'num rois: 0\n'
                      'processing <in>/f06.png\n'
                      'num rois: 0\n',
              'heatmaps': [],
              'files': {},
              'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                         ['frame_000000.png',
                          'frame_000001.png',
                          'frame_000002.png',
                          'frame_000003.png',
                          'frame_000004.png',
                          'frame_000005.png',
                          'frame_000006.png'])},
 'redact_shape': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                  'keywords': [('annotate', True),
                               ('draw', True),
                               ('redact', (('car',), 'pixelate', 16, 0)),
                               ('redact_shape', ('ellipse', 4))],
                  'thresholds': [0.0],
                  'said': 'processing <in>/f00.png\n'
                          'num rois: 0\n'
                          'processing <in>/f01.png\n'
                          'num rois: 0\n'
                          'processing <in>/f02.png\n'
                          'num rois: 0\n'
                          'processing <in>/f03.png\n'
                          'num rois: 0\n'
                          'processing <in>/f04.png\n'
                          'num rois: 0\n'
                          'processing <in>/f05.png\n'
                          'num rois: 0\n'
                          'processing <in>/f06.png\n'
                          'num rois: 0\n',
                  'heatmaps': [],
                  'files': {},
                  'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                             ['frame_000000.png',
                              'frame_000001.png',
                              'frame_000002.png',
                              'frame_000003.png',
                              'frame_000004.png',
                              'frame_000005.png',
                              'frame_000006.png'])},
 'redact_shape_box': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                      'keywords': [('annotate', True), ('draw', True), ('redact', (('car',), 'pixelate', 16, 0))],
                      'thresholds': [0.0],
                      'said': 'processing <in>/f00.png\n'
                              'num rois: 0\n'
                              'processing <in>/f01.png\n'
                              'num rois: 0\n'
                              'processing <in>/f02.png\n'
                              'num rois: 0\n'
                              'processing <in>/f03.png\n'
                              'num rois: 0\n'
                              'processing <in>/f04.png\n'
                              'num rois: 0\n'
                              'processing <in>/f05.png\n'
                              'num rois: 0\n'
                              'processing <in>/f06.png\n'
                              'num rois: 0\n',
                      'heatmaps': [],
                      'files': {},
                      'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                                 ['frame_000000.png',
                                  'frame_000001.png',
                                  'frame_000002.png',
                                  'frame_000003.png',
                                  'frame_000004.png',
                                  'frame_000005.png',
                                  'frame_000006.png'])},
 'det_threshold': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                   'keywords': [('annotate', True)],
                   'thresholds': [0.5],
                   'said': 'processing <in>/f00.png\n'
                           'num rois: 0\n'
                           'processing <in>/f01.png\n'
                           'num rois: 0\n'
                           'processing <in>/f02.png\n'
                           'num rois: 0\n'
                           'processing <in>/f03.png\n'
                           'num rois: 0\n'
                           'processing <in>/f04.png\n'
                           'num rois: 0\n'
                           'processing <in>/f05.png\n'
                           'num rois: 0\n'
                           'processing <in>/f06.png\n'
                           'num rois: 0\n',
                   'heatmaps': [],
                   'files': {},
                   'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                              ['frame_000000.png',
                               'frame_000001.png',
                               'frame_000002.png',
                               'frame_000003.png',
                               'frame_000004.png',
                               'frame_000005.png',
                               'frame_000006.png'])},
 'track_low': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
               'keywords': [('annotate', True), ('track', (30, 8, 0)), ('track_strong', 0.5)],
               'thresholds': [0.25],
               'said': 'processing <in>/f00.png\n'
                       'num rois: 0\n'
                       'processing <in>/f01.png\n'
                       'num rois: 0\n'
                       'processing <in>/f02.png\n'
                       'num rois: 0\n'
                       'processing <in>/f03.png\n'
                       'num rois: 0\n'
                       'processing <in>/f04.png\n'
                       'num rois: 0\n'
                       'processing <in>/f05.png\n'
                       'num rois: 0\n'
                       'processing <in>/f06.png\n'
                       'num rois: 0\n',
               'heatmaps': [],
               'files': {},
               'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                          ['frame_000000.png',
                           'frame_000001.png',
                           'frame_000002.png',
                           'frame_000003.png',
                           'frame_000004.png',
                           'frame_000005.png',
                           'frame_000006.png'])},
 'redact_region': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                   'keywords': [('annotate', True), ('redact_region', ((((0, 0), (4, 0), (4, 4)),), None, 'fill', 0, 0))],
                   'thresholds': [0.0],
                   'said': 'processing <in>/f00.png\n'
                           'num rois: 0\n'
                           'processing <in>/f01.png\n'
                           'num rois: 0\n'
                           'processing <in>/f02.png\n'
                           'num rois: 0\n'
                           'processing <in>/f03.png\n'
                           'num rois: 0\n'
                           'processing <in>/f04.png\n'
                           'num rois: 0\n'
                           'processing <in>/f05.png\n'
                           'num rois: 0\n'
                           'processing <in>/f06.png\n'
                           'num rois: 0\n'
                           'redact regions 8x6: 1 region, 12.5 % of the frame hidden\n'
                           'redact regions 8x8: 1 region, 9.4 % of the frame hidden\n',
                   'heatmaps': [],
                   'files': {},
                   'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                              ['frame_000000.png',
                               'frame_000001.png',
                               'frame_000002.png',
                               'frame_000003.png',
                               'frame_000004.png',
                               'frame_000005.png',
                               'frame_000006.png'])},
 'redact_moving': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                   'keywords': [('annotate', True), ('redact_moving', (24, 8, 4, 8, 0, 'show', (), 'pixelate', 16, 8, 10, 8))],
                   'thresholds': [0.0],
                   'said': 'processing <in>/f00.png\n'
                           'num rois: 0\n'
                           'processing <in>/f01.png\n'
                           'num rois: 0\n'
                           'processing <in>/f02.png\n'
                           'num rois: 0\n'
                           'processing <in>/f03.png\n'
                           'num rois: 0\n'
                           'processing <in>/f04.png\n'
                           'num rois: 0\n'
                           'processing <in>/f05.png\n'
                           'num rois: 0\n'
                           'processing <in>/f06.png\n'
                           'num rois: 0\n'
                           'moving net 8x6: 2 frames, mean 0.0 % hidden, peak 0.0 %\n'
                           'moving net 8x8: 5 frames, mean 0.0 % hidden, peak 0.0 %\n',
                   'heatmaps': [],
                   'files': {'moving.csv': 'frame,cells,covered\n1,0,0\n2,0,0\n3,0,0\n4,0,0\n5,0,0\n6,0,0\n7,0,0\n'},
                   'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                              ['frame_000000.png',
                               'frame_000001.png',
                               'frame_000002.png',
                               'frame_000003.png',
                               'frame_000004.png',
                               'frame_000005.png',
                               'frame_000006.png'])},
 'redact_moving_remove': {'passes': [(4, 4, 4), (1, 1, 1), (2, 2, 4)],
                          'keywords': [('annotate', True),
                                       ('redact_moving', (30, 8, 4, 8, 0, 'show', (), 'pixelate', 16, 4, 10, 8)),
                                       ('redact_region', ((((0, 0), (4, 0), (4, 4)),), None, 'fill', 0, 0)),
                                       ('remove', ('all', 4, 10, 8))],
                          'thresholds': [0.0],
                          'said': 'processing <in>/f00.png\n'
                                  'num rois: 0\n'
                                  'processing <in>/f01.png\n'
                                  'num rois: 0\n'
                                  'processing <in>/f02.png\n'
                                  'num rois: 0\n'
                                  'processing <in>/f03.png\n'
                                  'num rois: 0\n'
                                  'processing <in>/f04.png\n'
                                  'num rois: 0\n'
                                  'processing <in>/f05.png\n'
                                  'num rois: 0\n'
                                  'processing <in>/f06.png\n'
                                  'num rois: 0\n'
                                  'plate 8x6: 2 frames, 25.0 % known\n'
                                  'plate 8x8: 5 frames, 75.0 % known\n'
                                  'moving net 8x6: 2 frames, mean 0.0 % hidden, peak 0.0 %\n'
                                  'moving net 8x8: 5 frames, mean 0.0 % hidden, peak 0.0 %\n'
                                  'redact regions 8x6: 1 region, 12.5 % of the frame hidden\n'
                                  'redact regions 8x8: 1 region, 9.4 % of the frame hidden\n',
                          'heatmaps': [],
                          'files': {'plate_8x6.png': None, 'plate_8x8.png': None},
                          'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                                     ['frame_000000.png',
                                      'frame_000001.png',
                                      'frame_000002.png',
                                      'frame_000003.png',
                                      'frame_000004.png',
                                      'frame_000005.png',
                                      'frame_000006.png'])},
 'everything': {'passes': [(3, 5, 4), (1, 2, 1)],
                'keywords': [('annotate', True),
                             ('count', (((0, 0, 8, 8),), 'all', 3)),
                             ('detect_every', 2),
                             ('draw', True),
                             ('heat', ('all', 160, 0)),
                             ('out_size', ('scale', 2)),
                             ('redact', (('car',), 'pixelate', 16, 0)),
                             ('redact_moving', (24, 8, 4, 8, 0, 'show', (), 'pixelate', 16, 8, 10, 8)),
                             ('redact_region', ((((0, 0), (4, 0), (4, 4)),), None, 'fill', 0, 0)),
                             ('redact_shape', ('ellipse', 4)),
                             ('remove', (('car',), 8, 10, 8)),
                             ('track', (30, 8, 0)),
                             ('track_motion', 8),
                             ('track_reid', (25, 250)),
                             ('track_scene_cut', 40),
                             ('track_strong', 0.5),
                             ('track_trails', (16, 3)),
                             ('zone', ((((0, 0), (8, 0), (8, 8)),), 'all', 3, 0))],
                'thresholds': [0.25],
                'said': 'processing <in>/f00.png\n'
                        'num rois: 0\n'
                        'processing <in>/f01.png\n'
                        'num rois: 0\n'
                        'processing <in>/f02.png\n'
                        'num rois: 0\n'
                        'processing <in>/f03.png\n'
                        'num rois: 0\n'
                        'processing <in>/f04.png\n'
                        'num rois: 0\n'
                        'processing <in>/f05.png\n'
                        'num rois: 0\n'
                        'processing <in>/f06.png\n'
                        'num rois: 0\n'
                        'line 0: +2 -1\n'
                        "warning: 3 crossings did not fit their frames' lists: the counts file is short by that many rows; the totals "
                        'are exact\n'
                        'zone 0: visitors 4 peak 2 stays 2 mean dwell 4.5 frames\n'
                        "warning: 1 zone events did not fit their frames' lists: the zones file is short by that many rows; the totals "
                        'are exact\n'
                        're-identified: 0\n'
                        'plate 8x6: 2 frames, 25.0 % known\n'
                        'plate 8x8: 5 frames, 75.0 % known\n'
                        'moving net 8x6: 2 frames, mean 0.0 % hidden, peak 0.0 %\n'
                        'moving net 8x8: 5 frames, mean 0.0 % hidden, peak 0.0 %\n'
                        'redact regions 8x6: 1 region, 12.5 % of the frame hidden\n'
                        'redact regions 8x8: 1 region, 9.4 % of the frame hidden\n',
                'heatmaps': ['heat.png'],
                'files': {'counts.csv': 'frame,line,direction,id,cls\n',
                          'moving.csv': 'frame,cells,covered\n1,0,0\n2,0,0\n3,0,0\n4,0,0\n5,0,0\n6,0,0\n7,0,0\n',
                          'plate_8x6.png': None,
                          'plate_8x8.png': None,
                          'reid.csv': 'frame,id,tracker_id,cls,distance,gap\n',
                          'zones.csv': 'frame,zone,kind,id,cls,dwell\n',
                          'tracks_out': ''},
                'frames': (['f00.png', 'f01.png', 'f02.png', 'f03.png', 'f04.png', 'f05.png', 'f06.png'],
                           ['frame_000000.png',
                            'frame_000001.png',
                            'frame_000002.png',
                            'frame_000003.png',
                            'frame_000004.png',
                            'frame_000005.png',
                            'frame_000006.png'])}}
ONE_FRAME = {'plain': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True)])], 'thresholds': [0.0], 'said': 'num rois: 0\n', 'files': {}},
 'redact': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('redact', (('car',), 'pixelate', 16, 0))])],
            'thresholds': [0.0],
            'said': 'num rois: 0\n',
            'files': {}},
 'draw': {'calls': [(1, 1, 1, [('annotate', True), ('draw', False)])], 'thresholds': [0.0], 'said': 'num rois: 0\n', 'files': {}},
 'track': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('track', (30, 8, 0))])],
           'thresholds': [0.0],
           'said': 'num rois: 0\n',
           'files': {'tracks_out': ''}},
 'track_motion': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('track', (30, 8, 0)), ('track_motion', 8)])],
                  'thresholds': [0.0],
                  'said': 'num rois: 0\n',
                  'files': {}},
 'track_scene_cut': {'calls': [(1,
                                1,
                                1,
                                [('annotate', True),
                                 ('draw', True),
                                 ('track', (30, 8, 0)),
                                 ('track_motion', 8),
                                 ('track_scene_cut', 40)])],
                     'thresholds': [0.0],
                     'said': 'num rois: 0\n',
                     'files': {}},
 'track_trails': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('track', (30, 8, 0)), ('track_trails', (16, 3))])],
                  'thresholds': [0.0],
                  'said': 'num rois: 0\n',
                  'files': {}},
 'heatmap': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('heat', ('all', 160, 0))])],
             'thresholds': [0.0],
             'said': 'num rois: 0\n',
             'files': {}},
 'count': {'calls': [(1, 1, 1, [('annotate', True), ('count', (((0, 0, 8, 8),), 'all', 3)), ('draw', True), ('track', (30, 8, 0))])],
           'thresholds': [0.0],
           'said': 'num rois: 0\n',
           'files': {'counts_out': ''}},
 'zone': {'calls': [(1,
                     1,
                     1,
                     [('annotate', True),
                      ('draw', True),
                      ('track', (30, 8, 0)),
                      ('zone', ((((0, 0), (8, 0), (8, 8)),), 'all', 3, 0))])],
          'thresholds': [0.0],
          'said': 'num rois: 0\n',
          'files': {'zones_out': ''}},
 'remove': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('remove', (('car',), 8, 10, 8))])],
            'thresholds': [0.0],
            'said': 'num rois: 0\n',
            'files': {}},
 'track_reid': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('track', (30, 8, 0)), ('track_reid', (25, 250))])],
                'thresholds': [0.0],
                'said': 'num rois: 0\n',
                'files': {'reid_out': ''}},
 'post': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True)])], 'thresholds': [0.0], 'said': 'num rois: 0\n', 'files': {}},
 'out_size': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('out_size', ('scale', 2))])],
              'thresholds': [0.0],
              'said': 'num rois: 0\n',
              'files': {}},
 'redact_shape': {'calls': [(1,
                             1,
                             1,
                             [('annotate', True),
                              ('draw', True),
                              ('redact', (('car',), 'pixelate', 16, 0)),
                              ('redact_shape', ('ellipse', 4))])],
                  'thresholds': [0.0],
                  'said': 'num rois: 0\n',
                  'files': {}},
 'redact_shape_box': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('redact', (('car',), 'pixelate', 16, 0))])],
                      'thresholds': [0.0],
                      'said': 'num rois: 0\n',
                      'files': {}},
 'det_threshold': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True)])],
                   'thresholds': [0.5],
                   'said': 'num rois: 0\n',
                   'files': {}},
 'track_low': {'calls': [(1, 1, 1, [('annotate', True), ('draw', True), ('track', (30, 8, 0)), ('track_strong', 0.5)])],
               'thresholds': [0.25],
               'said': 'num rois: 0\n',
               'files': {}},
 'redact_region': {'calls': [(1,
                              1,
                              1,
                              [('annotate', True),
                               ('draw', True),
                               ('redact_region', ((((0, 0), (4, 0), (4, 4)),), None, 'fill', 0, 0))])],
                   'thresholds': [0.0],
                   'said': 'num rois: 0\n',
                   'files': {}},
 'redact_moving': {'calls': [(1,
                              1,
                              1,
                              [('annotate', True),
                               ('draw', True),
                               ('redact_moving', (24, 8, 4, 8, 0, 'show', (), 'pixelate', 16, 8, 10, 8))])],
                   'thresholds': [0.0],
                   'said': 'num rois: 0\n',
                   'files': {}},
 'redact_moving_remove': {'calls': [(1,
                                     1,
                                     1,
                                     [('annotate', True),
                                      ('draw', True),
                                      ('redact_moving', (30, 8, 4, 8, 0, 'show', (), 'pixelate', 16, 4, 10, 8)),
                                      ('redact_region', ((((0, 0), (4, 0), (4, 4)),), None, 'fill', 0, 0)),
                                      ('remove', ('all', 4, 10, 8))])],
                          'thresholds': [0.0],
                          'said': 'num rois: 0\n',
                          'files': {}}}
EAGER = {'plain': {'asked': [[('det_threshold', 0.0), ('post', None), ('stride', 16)],
                     [('det_threshold', 0.0), ('post', None), ('stride', 16)]],
           'said': 'processing <in>/f00.png\nprocessing <in>/f01.png\n',
           'frames': ['f00.png', 'f01.png']},
 'redact': {'asked': [[('det_threshold', 0.0), ('post', None), ('stride', 16)],
                      [('det_threshold', 0.0), ('post', None), ('stride', 16)]],
            'said': 'processing <in>/f00.png\nprocessing <in>/f01.png\n',
            'frames': ['f00.png', 'f01.png']},
 'draw': {'asked': [[('det_threshold', 0.0), ('post', None), ('stride', 16)], [('det_threshold', 0.0), ('post', None), ('stride', 16)]],
          'said': 'processing <in>/f00.png\nprocessing <in>/f01.png\n',
          'frames': ['f00.png', 'f01.png']},
 'post': {'asked': [[('det_threshold', 0.0), ('post', ('soft_linear', 0.5, 0.5, None, None)), ('stride', 16)],
                    [('det_threshold', 0.0), ('post', ('soft_linear', 0.5, 0.5, None, None)), ('stride', 16)]],
          'said': 'processing <in>/f00.png\nprocessing <in>/f01.png\n',
          'frames': ['f00.png', 'f01.png']},
 'det_threshold': {'asked': [[('det_threshold', 0.5), ('post', None), ('stride', 16)],
                             [('det_threshold', 0.5), ('post', None), ('stride', 16)]],
                   'said': 'processing <in>/f00.png\nprocessing <in>/f01.png\n',
                   'frames': ['f00.png', 'f01.png']}}
REFUSED = {'motion_needs_track': {'annotate_images': ('ValueError',
                                            'track_motion=8 moves the boxes of the tracker: it needs track=(thr, hold, grow)'),
                        'annotate_stream': ('ValueError',
                                            'track_motion=8 moves the boxes of the tracker: it needs track=(thr, hold, grow)'),
                        'get_annotated_frame': ('ValueError',
                                                'track_motion=8 moves the boxes of the tracker: it needs track=(thr, hold, grow)'),
                        'draw_eager': ('ValueError',
                                       'track_motion=8 moves the boxes of the tracker: it needs track=(thr, hold, grow)')},
 'lookback_needs_track': {'annotate_images': ('ValueError',
                                              "track_lookback=2 hides the tracker's new tracks in earlier frames: it needs track=(thr, "
                                              'hold, grow)'),
                          'annotate_stream': ('ValueError',
                                              "track_lookback=2 hides the tracker's new tracks in earlier frames: it needs track=(thr, "
                                              'hold, grow)'),
                          'get_annotated_frame': ('ValueError',
                                                  'track_lookback=2 delays the output: get_annotated_frame returns its frame at once '
                                                  'and cannot; use annotate_images or annotate_stream')},
 'every_needs_motion': {'annotate_images': ('ValueError',
                                            'detect_every=2 follows the tracks by block matching between two detected frames: it needs '
                                            'track=(thr, hold, grow) and track_motion=R'),
                        'annotate_stream': ('ValueError',
                                            'detect_every=2 follows the tracks by block matching between two detected frames: it needs '
                                            'track=(thr, hold, grow) and track_motion=R'),
                        'get_annotated_frame': ('ValueError',
                                                'detect_every=2 runs the detector once per pass of several frames: get_annotated_frame '
                                                'detects its one frame and cannot; use annotate_images or annotate_stream')},
 'every_with_lookback': {'annotate_images': ('ValueError',
                                             'detect_every=2 together with track_lookback=2 is not supported: the look-back window '
                                             'keeps one tracked buffer per detected frame'),
                         'annotate_stream': ('ValueError',
                                             'detect_every=2 together with track_lookback=2 is not supported: the look-back window '
                                             'keeps one tracked buffer per detected frame'),
                         'get_annotated_frame': ('ValueError',
                                                 'detect_every=2 runs the detector once per pass of several frames: '
                                                 'get_annotated_frame detects its one frame and cannot; use annotate_images or '
                                                 'annotate_stream')},
 'backtrack_needs_every': {'annotate_images': ('ValueError',
                                               'track_backtrack=2 follows the tracks of a detected frame back over the frames between '
                                               'two detections: it needs track=(thr, hold, grow), track_motion=R and detect_every=K'),
                           'annotate_stream': ('ValueError',
                                               'track_backtrack=2 follows the tracks of a detected frame back over the frames between '
                                               'two detections: it needs track=(thr, hold, grow), track_motion=R and detect_every=K'),
                           'get_annotated_frame': ('ValueError',
                                                   'track_backtrack=2 delays the output: get_annotated_frame returns its frame at once '
                                                   'and cannot; use annotate_images or annotate_stream')},
 'backtrack_with_lookback': {'annotate_images': ('ValueError',
                                                 'track_backtrack=2 together with track_lookback=2 is not supported: the back-track '
                                                 'rule hides a new track in the earlier frames itself'),
                             'annotate_stream': ('ValueError',
                                                 'track_backtrack=2 together with track_lookback=2 is not supported: the back-track '
                                                 'rule hides a new track in the earlier frames itself'),
                             'get_annotated_frame': ('ValueError',
                                                     'track_backtrack=2 delays the output: get_annotated_frame returns its frame at '
                                                     'once and cannot; use annotate_images or annotate_stream')},
 'cut_needs_motion': {'annotate_images': ('ValueError',
                                          'track_scene_cut=40 compares every frame with the frame the block match keeps: it needs '
                                          'track=(thr, hold, grow) and track_motion=R'),
                      'annotate_stream': ('ValueError',
                                          'track_scene_cut=40 compares every frame with the frame the block match keeps: it needs '
                                          'track=(thr, hold, grow) and track_motion=R'),
                      'get_annotated_frame': ('ValueError',
                                              'track_scene_cut=40 compares every frame with the frame the block match keeps: it needs '
                                              'track=(thr, hold, grow) and track_motion=R'),
                      'draw_eager': ('ValueError',
                                     'track_scene_cut=40 compares every frame with the frame the block match keeps: it needs '
                                     'track=(thr, hold, grow) and track_motion=R')},
 'cut_with_lookback': {'annotate_images': ('ValueError',
                                           'track_scene_cut=40 together with track_lookback=2 is not supported: a backward chain would '
                                           'have to stop at a cut'),
                       'annotate_stream': ('ValueError',
                                           'track_scene_cut=40 together with track_lookback=2 is not supported: a backward chain would '
                                           'have to stop at a cut'),
                       'get_annotated_frame': ('ValueError',
                                               'track_lookback=2 delays the output: get_annotated_frame returns its frame at once and '
                                               'cannot; use annotate_images or annotate_stream')},
 'cut_with_backtrack': {'annotate_images': ('ValueError',
                                            'track_scene_cut=40 together with track_backtrack=2 is not supported: a backward chain '
                                            'would have to stop at a cut'),
                        'annotate_stream': ('ValueError',
                                            'track_scene_cut=40 together with track_backtrack=2 is not supported: a backward chain '
                                            'would have to stop at a cut'),
                        'get_annotated_frame': ('ValueError',
                                                'detect_every=2 runs the detector once per pass of several frames: get_annotated_frame '
                                                'detects its one frame and cannot; use annotate_images or annotate_stream')},
 'trails_need_track': {'annotate_images': ('ValueError',
                                           "track_trails=(16, 3) draws the paths of the tracker's ids: it needs track=(thr, hold, "
                                           'grow)'),
                       'annotate_stream': ('ValueError',
                                           "track_trails=(16, 3) draws the paths of the tracker's ids: it needs track=(thr, hold, "
                                           'grow)'),
                       'get_annotated_frame': ('ValueError',
                                               "track_trails=(16, 3) draws the paths of the tracker's ids: it needs track=(thr, hold, "
                                               'grow)'),
                       'draw_eager': ('ValueError',
                                      "track_trails=(16, 3) draws the paths of the tracker's ids: it needs track=(thr, hold, grow)")},
 'trails_with_no_draw': {'annotate_images': ('ValueError',
                                             'track_trails=(16, 3) together with draw=False is not supported: a run that draws nothing '
                                             'draws no trails'),
                         'annotate_stream': ('ValueError',
                                             'track_trails=(16, 3) together with draw=False is not supported: a run that draws nothing '
                                             'draws no trails'),
                         'get_annotated_frame': ('ValueError',
                                                 'track_trails=(16, 3) together with draw=False is not supported: a run that draws '
                                                 'nothing draws no trails'),
                         'draw_eager': ('ValueError',
                                        'track_trails=(16, 3) together with draw=False is not supported: a run that draws nothing '
                                        'draws no trails')},
 'heatmap_out_needs_heatmap': {'annotate_images': ('ValueError',
                                                   "heatmap_out='heat.png' is where the heat map is written: it needs "
                                                   'heatmap=(classes, alpha, decay)'),
                               'annotate_stream': ('ValueError',
                                                   "heatmap_out='heat.png' is where the heat map is written: it needs "
                                                   'heatmap=(classes, alpha, decay)')},
 'heatmap_out_not_png': {'annotate_images': ('ValueError',
                                             "heatmap_out='heat.csv': the map is written as an 8-bit grey PNG, a path that ends in "
                                             '.png'),
                         'annotate_stream': ('ValueError',
                                             "heatmap_out='heat.csv': the map is written as an 8-bit grey PNG, a path that ends in "
                                             '.png')},
 'count_needs_track': {'annotate_images': ('ValueError',
                                           "count=(((0, 0, 8, 8),), 'all', None) counts the tracker's ids as they cross a line: it "
                                           'needs track=(thr, hold, grow)'),
                       'annotate_stream': ('ValueError',
                                           "count=(((0, 0, 8, 8),), 'all', None) counts the tracker's ids as they cross a line: it "
                                           'needs track=(thr, hold, grow)'),
                       'get_annotated_frame': ('ValueError',
                                               "count=(((0, 0, 8, 8),), 'all', None) counts the tracker's ids as they cross a line: it "
                                               'needs track=(thr, hold, grow)'),
                       'draw_eager': ('ValueError',
                                      "count=(((0, 0, 8, 8),), 'all', None) counts the tracker's ids as they cross a line: it needs "
                                      'track=(thr, hold, grow)')},
 'counts_out_needs_count': {'annotate_images': ('ValueError',
                                                "counts_out='counts.csv' is where the crossings are written: it needs count=(lines, "
                                                'classes, width)'),
                            'annotate_stream': ('ValueError',
                                                "counts_out='counts.csv' is where the crossings are written: it needs count=(lines, "
                                                'classes, width)'),
                            'get_annotated_frame': ('ValueError',
                                                    'counts_out is where the crossings are written: it needs count=(lines, classes, '
                                                    'width)')},
 'zone_needs_track': {'annotate_images': ('ValueError',
                                          "zone=((((0, 0), (8, 0), (8, 8)),), 'all', None, None) tests the tracker's ids against the "
                                          'zones: it needs track=(thr, hold, grow)'),
                      'annotate_stream': ('ValueError',
                                          "zone=((((0, 0), (8, 0), (8, 8)),), 'all', None, None) tests the tracker's ids against the "
                                          'zones: it needs track=(thr, hold, grow)'),
                      'get_annotated_frame': ('ValueError',
                                              "zone=((((0, 0), (8, 0), (8, 8)),), 'all', None, None) tests the tracker's ids against "
                                              'the zones: it needs track=(thr, hold, grow)'),
                      'draw_eager': ('ValueError',
                                     "zone=((((0, 0), (8, 0), (8, 8)),), 'all', None, None) tests the tracker's ids against the zones: "
                                     'it needs track=(thr, hold, grow)')},
 'zones_out_needs_zone': {'annotate_images': ('ValueError',
                                              "zones_out='zones.csv' is where the zone events are written: it needs zone=(zones, "
                                              'classes, width, anchor)'),
                          'annotate_stream': ('ValueError',
                                              "zones_out='zones.csv' is where the zone events are written: it needs zone=(zones, "
                                              'classes, width, anchor)'),
                          'get_annotated_frame': ('ValueError',
                                                  'zones_out is where the zone events are written: it needs zone=(zones, classes, '
                                                  'width, anchor)')},
 'remove_unknown_class': {'annotate_images': ('ValueError', 'remove: unknown class name \'cat\'; the classes are: car (or "all")'),
                          'annotate_stream': ('ValueError', 'remove: unknown class name \'cat\'; the classes are: car (or "all")'),
                          'get_annotated_frame': None},
 'plate_out_needs_remove': {'annotate_images': ('ValueError',
                                                "plate_out='plate.png' is where the background plate is written: it needs "
                                                'remove=(classes, settle, tol, margin)'),
                            'annotate_stream': ('ValueError',
                                                "plate_out='plate.png' is where the background plate is written: it needs "
                                                'remove=(classes, settle, tol, margin)')},
 'reid_needs_track': {'annotate_images': ('ValueError',
                                          "track_reid=(25, None) gives the tracker's ids back: it needs track=(thr, hold, grow)"),
                      'annotate_stream': ('ValueError',
                                          "track_reid=(25, None) gives the tracker's ids back: it needs track=(thr, hold, grow)"),
                      'get_annotated_frame': ('ValueError',
                                              "track_reid=(25, None) gives the tracker's ids back: it needs track=(thr, hold, grow)"),
                      'draw_eager': ('ValueError',
                                     "track_reid=(25, None) gives the tracker's ids back: it needs track=(thr, hold, grow)")},
 'reid_out_needs_reid': {'annotate_images': ('ValueError',
                                             "reid_out='reid.csv' is where the re-identifications are written: it needs "
                                             'track_reid=(pct, keep)'),
                         'annotate_stream': ('ValueError',
                                             "reid_out='reid.csv' is where the re-identifications are written: it needs "
                                             'track_reid=(pct, keep)'),
                         'get_annotated_frame': ('ValueError',
                                                 'reid_out is where the re-identifications are written: it needs track_reid=(pct, '
                                                 'keep)')},
 'reid_with_lookback': {'annotate_images': ('ValueError',
                                            'track_reid=(25, 250) together with track_lookback= / track_backtrack= is not supported: '
                                            "the window of a delayed pass holds the tracker's own ids"),
                        'annotate_stream': ('ValueError',
                                            'track_reid=(25, 250) together with track_lookback= / track_backtrack= is not supported: '
                                            "the window of a delayed pass holds the tracker's own ids"),
                        'get_annotated_frame': ('ValueError', 'track_reid=(25, 250) together with track_lookback= is not supported')},
 'reid_with_backtrack': {'annotate_images': ('ValueError',
                                             'track_reid=(25, 250) together with track_lookback= / track_backtrack= is not supported: '
                                             "the window of a delayed pass holds the tracker's own ids"),
                         'annotate_stream': ('ValueError',
                                             'track_reid=(25, 250) together with track_lookback= / track_backtrack= is not supported: '
                                             "the window of a delayed pass holds the tracker's own ids"),
                         'get_annotated_frame': ('ValueError',
                                                 'detect_every=2 runs the detector once per pass of several frames: '
                                                 'get_annotated_frame detects its one frame and cannot; use annotate_images or '
                                                 'annotate_stream')},
 'shape_needs_redact': {'annotate_images': ('ValueError',
                                            "redact_shape=('ellipse', 4) shapes the redaction: it needs redact=(classes, mode, size, "
                                            'margin)'),
                        'annotate_stream': ('ValueError',
                                            "redact_shape=('ellipse', 4) shapes the redaction: it needs redact=(classes, mode, size, "
                                            'margin)'),
                        'get_annotated_frame': ('ValueError',
                                                "redact_shape=('ellipse', 4) shapes the redaction: it needs redact=(classes, mode, "
                                                'size, margin)'),
                        'draw_eager': ('ValueError',
                                       "redact_shape=('ellipse', 4) shapes the redaction: it needs redact=(classes, mode, size, "
                                       'margin)')},
 'low_needs_track': {'annotate_images': ('ValueError', 'track low=0.25 needs tracking (track): a weak row can only continue a track'),
                     'annotate_stream': ('ValueError', 'track low=0.25 needs tracking (track): a weak row can only continue a track'),
                     'get_annotated_frame': ('ValueError',
                                             'track low=0.25 needs tracking (track): a weak row can only continue a track')},
 'low_not_under_threshold': {'annotate_images': ('ValueError',
                                                 'track low=0.5 must be below det threshold=0.25: the rows between the two are the '
                                                 'weak ones'),
                             'annotate_stream': ('ValueError',
                                                 'track low=0.5 must be below det threshold=0.25: the rows between the two are the '
                                                 'weak ones'),
                             'get_annotated_frame': ('ValueError',
                                                     'track low=0.5 must be below det threshold=0.25: the rows between the two are the '
                                                     'weak ones')},
 'moving_out_needs_moving': {'annotate_images': ('ValueError',
                                                 "moving_out='moving.csv' is where the moving net's counts are written: it needs "
                                                 'redact_moving='),
                             'annotate_stream': ('ValueError',
                                                 "moving_out='moving.csv' is where the moving net's counts are written: it needs "
                                                 'redact_moving='),
                             'get_annotated_frame': None},
 'moving_plate_differs': {'annotate_images': ('ValueError',
                                              'redact_moving: settle=3, but remove= says 4: a pass has one plate update, state it '
                                              'once'),
                          'annotate_stream': ('ValueError',
                                              'redact_moving: settle=3, but remove= says 4: a pass has one plate update, state it '
                                              'once'),
                          'get_annotated_frame': ('ValueError',
                                                  'redact_moving: settle=3, but remove= says 4: a pass has one plate update, state it '
                                                  'once'),
                          'draw_eager': ('ValueError',
                                         'redact_moving: settle=3, but remove= says 4: a pass has one plate update, state it once')},
 'lookback_on_one_frame': {'annotate_images': None,
                           'annotate_stream': None,
                           'get_annotated_frame': ('ValueError',
                                                   'track_lookback=2 delays the output: get_annotated_frame returns its frame at once '
                                                   'and cannot; use annotate_images or annotate_stream')},
 'every_on_one_frame': {'annotate_images': None,
                        'annotate_stream': None,
                        'get_annotated_frame': ('ValueError',
                                                'detect_every=2 runs the detector once per pass of several frames: get_annotated_frame '
                                                'detects its one frame and cannot; use annotate_images or annotate_stream')},
 'backtrack_on_one_frame': {'annotate_images': None,
                            'annotate_stream': None,
                            'get_annotated_frame': ('ValueError',
                                                    'detect_every=2 runs the detector once per pass of several frames: '
                                                    'get_annotated_frame detects its one frame and cannot; use annotate_images or '
                                                    'annotate_stream')},
 'two_need_track': {'annotate_images': ('ValueError',
                                        'track_motion=8 moves the boxes of the tracker: it needs track=(thr, hold, grow)'),
                    'annotate_stream': ('ValueError',
                                        'track_motion=8 moves the boxes of the tracker: it needs track=(thr, hold, grow)'),
                    'get_annotated_frame': ('ValueError',
                                            "track_reid=(25, None) gives the tracker's ids back: it needs track=(thr, hold, grow)"),
                    'draw_eager': ('ValueError',
                                   "track_reid=(25, None) gives the tracker's ids back: it needs track=(thr, hold, grow)")},
 'two_outputs_and_a_shape': {'annotate_images': ('ValueError',
                                                 "post-process mode 'no such mode': one of hard, soft_linear, soft_gaussian"),
                             'annotate_stream': ('ValueError',
                                                 "post-process mode 'no such mode': one of hard, soft_linear, soft_gaussian"),
                             'get_annotated_frame': ('ValueError',
                                                     "post-process mode 'no such mode': one of hard, soft_linear, soft_gaussian")}}
HANDED_ON = {'bare': [('annotate_images',
           [],
           [('draw', True),
            ('frame_format', 'png'),
            ('image_filenames', ['f00.png']),
            ('input_dir', '<tmp>/in'),
            ('jpeg_encoder', 'host'),
            ('jpeg_huffman', 'standard'),
            ('jpeg_subsampling', 444),
            ('out_dir', '<tmp>/out'),
            ('png_compress', 'runs'),
            ('png_encoder', 'host'),
            ('resize_max', 1000),
            ('resize_min', 600)])],
 'every_option': [('annotate_images',
                   [],
                   [('count', (((0, 0, 8, 8),), ('car',), 2)),
                    ('counts_out', '<tmp>/counts.csv'),
                    ('det_threshold', 0.5),
                    ('detect_every', 2),
                    ('draw', True),
                    ('frame_format', 'png'),
                    ('heatmap', ('all', 100, 2)),
                    ('heatmap_out', '<tmp>/heat.png'),
                    ('image_filenames', ['f00.png']),
                    ('input_dir', '<tmp>/in'),
                    ('jpeg_encoder', 'host'),
                    ('jpeg_huffman', 'standard'),
                    ('jpeg_subsampling', 444),
                    ('moving_out', '<tmp>/moving.csv'),
                    ('out_dir', '<tmp>/out'),
                    ('out_size', ('scale', 2)),
                    ('plate_out', '<tmp>/plate.png'),
                    ('png_compress', 'runs'),
                    ('png_encoder', 'host'),
                    ('post', ('soft_linear', 0.5, 0.5, None, None)),
                    ('redact', (('car',), 'blur', 5, 2)),
                    ('redact_moving', (30, 4, 2, 3, 1, 'hide', ('car',), 'fill', 0, 4, 5, 3)),
                    ('redact_region', ((((0, 0), (4, 0), (4, 4)),), None, 'blur', 3, 2)),
                    ('redact_shape', ('ellipse', 4)),
                    ('reid_out', '<tmp>/reid.csv'),
                    ('remove', (('person',), 4, 5, 3)),
                    ('resize_max', 1000),
                    ('resize_min', 600),
                    ('track', (40, 4, 1)),
                    ('track_low', 0.25),
                    ('track_motion', 8),
                    ('track_reid', (25, 100)),
                    ('track_scene_cut', 40),
                    ('track_trails', (16, 5)),
                    ('tracks_out', '<file tracks.txt>'),
                    ('zone', ((((0, 0), (8, 0), (8, 8)),), ('car',), 2, 1)),
                    ('zones_out', '<tmp>/zones.csv')])],
 'every_option_to_a_video': [('annotate_stream',
                              ['<frames>', '<y4m writer 4x4>', 600, 1000],
                              [('count', (((0, 0, 8, 8),), ('car',), 2)),
                               ('counts_out', '<tmp>/counts.csv'),
                               ('det_threshold', 0.5),
                               ('detect_every', 2),
                               ('draw', True),
                               ('heatmap', ('all', 100, 2)),
                               ('heatmap_out', '<tmp>/heat.png'),
                               ('moving_out', '<tmp>/moving.csv'),
                               ('out_size', ('scale', 2)),
                               ('plate_out', '<tmp>/plate.png'),
                               ('post', ('soft_linear', 0.5, 0.5, None, None)),
                               ('redact', (('car',), 'blur', 5, 2)),
                               ('redact_moving', (30, 4, 2, 3, 1, 'hide', ('car',), 'fill', 0, 4, 5, 3)),
                               ('redact_region', ((((0, 0), (4, 0), (4, 4)),), None, 'blur', 3, 2)),
                               ('redact_shape', ('ellipse', 4)),
                               ('reid_out', '<tmp>/reid.csv'),
                               ('remove', (('person',), 4, 5, 3)),
                               ('track', (40, 4, 1)),
                               ('track_low', 0.25),
                               ('track_motion', 8),
                               ('track_reid', (25, 100)),
                               ('track_scene_cut', 40),
                               ('track_trails', (16, 5)),
                               ('tracks_out', '<file tracks.txt>'),
                               ('zone', ((((0, 0), (8, 0), (8, 8)),), ('car',), 2, 1)),
                               ('zones_out', '<tmp>/zones.csv')])],
 'no_draw_and_lookback': [('annotate_images',
                           [],
                           [('draw', False),
                            ('frame_format', 'png'),
                            ('image_filenames', ['f00.png']),
                            ('input_dir', '<tmp>/in'),
                            ('jpeg_encoder', 'host'),
                            ('jpeg_huffman', 'standard'),
                            ('jpeg_subsampling', 444),
                            ('out_dir', '<tmp>/out'),
                            ('png_compress', 'runs'),
                            ('png_encoder', 'host'),
                            ('resize_max', 1000),
                            ('resize_min', 600),
                            ('track', (30, 8, 0)),
                            ('track_lookback', 0)])],
 'backtrack': [('annotate_images',
                [],
                [('detect_every', 3),
                 ('draw', True),
                 ('frame_format', 'png'),
                 ('image_filenames', ['f00.png']),
                 ('input_dir', '<tmp>/in'),
                 ('jpeg_encoder', 'host'),
                 ('jpeg_huffman', 'standard'),
                 ('jpeg_subsampling', 444),
                 ('out_dir', '<tmp>/out'),
                 ('png_compress', 'runs'),
                 ('png_encoder', 'host'),
                 ('resize_max', 1000),
                 ('resize_min', 600),
                 ('track', (30, 8, 0)),
                 ('track_backtrack', 0),
                 ('track_motion', 4)])]}
