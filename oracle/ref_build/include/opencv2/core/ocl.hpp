// TEST INFRASTRUCTURE (oracle/ref_build only): everything the stand-in has is in opencv2/core.hpp.
#pragma once
#include "opencv2/core.hpp"
