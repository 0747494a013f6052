// The geometry of a device environment's frame and of the launch that writes it (contract: include/drqv2_hip.h, "device
// environment"): shared by the skeleton of the tasks (vecenv_task.h) and by the distractions drawn over their frames
// (vecdistract.hip).
#pragma once
#include "common.h"

static constexpr int kSide = 84;
static constexpr int kPlane = kSide * kSide;             // 7,056 bytes = 441 x 16
static constexpr int kFrame = 3 * kPlane;                // 21,168 bytes = 1,323 x 16
static constexpr int kPieces = kFrame / 16;
static constexpr int kThreads = 256;
