"""The drop-in (fastest_image_pattern_matching_amd/dropin/TemplateMatcher_fpm.cpp) compiled and linked with a driver
that takes the class's member functions as the reference application does and prints the sizes of the types that cross
the interface -- CPU only, no GPU call is made.

The reference's own headers (include/TemplateMatcher.h, DataStructures.h) need OpenCV and Qt and are not part of this
repository, so the build uses the header excerpts of tests/dropin, where tests/dropin/opencv2/opencv.hpp stands in for
OpenCV with OpenCV 4.x's data layouts.  What is checked is what those headers can show: the drop-in defines the members
with the reference's signatures (the driver links), the stand-in's types have OpenCV 4.x's sizes on x86-64, and
s_SingleTargetMatch, which fpm_result must equal byte for byte, has the reference's 96 bytes.  sizeof(s_TemplData) and
sizeof(TemplateMatcher) of the reference build (168 and 352: the excerpt leaves out members the drop-in never touches)
can only be checked against the reference's unmodified headers, on a host that has them.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# OpenCV 4.x, x86-64: sizeof(cv::Mat) 96, cv::Rect 16, cv::Scalar 32, cv::RotatedRect 20, cv::Point2d 16
# s_SingleTargetMatch: 5 cv::Point2d 80 + 2 double 16 = 96
EXPECTED = {"cv::Mat": 96, "cv::Rect": 16, "cv::Scalar": 32, "cv::RotatedRect": 20, "cv::Point2d": 16,
            "s_SingleTargetMatch": 96}

DRIVER = r"""
#include "TemplateMatcher.h"
#include <cstdio>
int main() {
    // the class as the header declares it, defined by the drop-in; nothing is constructed (no GPU here)
    bool (TemplateMatcher::*learn)(const cv::Mat&) = &TemplateMatcher::learnPattern;
    std::vector<s_SingleTargetMatch> (TemplateMatcher::*match)(const cv::Mat&) = &TemplateMatcher::match;
    void (TemplateMatcher::*rect)(const cv::Rect&) = &TemplateMatcher::setUserDefinedRect;
    (void)learn; (void)match; (void)rect;
    std::printf("cv::Mat %zu\ncv::Rect %zu\ncv::Scalar %zu\ncv::RotatedRect %zu\ncv::Point2d %zu\n", sizeof(cv::Mat),
                sizeof(cv::Rect), sizeof(cv::Scalar), sizeof(cv::RotatedRect), sizeof(cv::Point2d));
    std::printf("s_SingleTargetMatch %zu\n", sizeof(s_SingleTargetMatch));
    return 0;
}
"""


def test_dropin_layout_with_standin_headers(tmp_path):
    lib = os.path.join(REPO, "fastest_image_pattern_matching_amd", "lib")
    assert os.path.exists(os.path.join(lib, "libfpm_hip.so")), "libfpm_hip.so not built"
    drv = tmp_path / "driver.cpp"
    drv.write_text(DRIVER)
    exe = tmp_path / "driver"
    inc = os.path.join(REPO, "tests", "dropin")
    dropin = os.path.join(REPO, "fastest_image_pattern_matching_amd", "dropin", "TemplateMatcher_fpm.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-fPIC", "-I" + inc, "-I" + os.path.join(REPO, "include"),
           dropin, str(drv), "-L" + lib, "-lfpm_hip", "-Wl,-rpath," + lib, "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out =subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    sizes = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert sizes == EXPECTED
