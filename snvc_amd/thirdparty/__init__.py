"""Stand-ins for the reference's ``snvc.thirdparty`` package, of which the release holds no file: ``oriented_iou_loss`` serves
the import line the reference left commented out (snvc/models/loss3d.py:12)."""
