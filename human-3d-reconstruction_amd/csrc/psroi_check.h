// The argument checks of the PS-ROI pooling entry points and their texts: defined in csrc/psroi.hip, used by the forward and by the
// backward (csrc/psroi_bwd.hip).  Each returns H3D_OK or records the error and returns its code.
#pragma once

int psroi_check_common(const char *what, int B, int C, int H, int W, int R, int output_dim, int group_size, int P, int part, int spp);
int psroi_check_trans(const char *what, int channels_trans, int output_dim, int *ncls);
int psroi_check_limits(const char *what, int P, int part, int spp);
