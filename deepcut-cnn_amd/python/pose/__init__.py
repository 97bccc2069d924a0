from .people import MIRROR_MPII14, SKELETON_MPII14, estimate_people, track_people, draw_people, draw_heatmap, redact_people, label_people, people_boxes, HEAD_MPII14  # noqa: F401
