// nuslam's usage of rigid2d::EKF_SLAM (slam.cpp:213,217,259,380,428,433-434; unknown_data_assoc.cpp:415) as one
// translation unit: oracle/Makefile compiles it against the drop-in shim header and the reference's real rigid2d.hpp
// into oracle/_ref/nuslam_caller.o, which tests/test_shim.py checks.
#include "rigid2d/ekf_slam.hpp"
struct Node {
    rigid2d::EKF_SLAM slam_agent;              // slam.cpp:213
    mat sensor_reading = zeros<mat>(40, 1);    // slam.cpp:217,259 (bare `mat`: the header's using-directive)
    std::vector<bool> visible_list = std::vector<bool>(20, false), known_list = std::vector<bool>(20, false);
    std::vector<rigid2d::Vector2D> scan_measures;
    void tick(const rigid2d::Twist2D& tw) {
        slam_agent = rigid2d::EKF_SLAM(20);    // slam.cpp:428
        slam_agent.prediction(tw);             // slam.cpp:433
        slam_agent.measurement(sensor_reading, visible_list, known_list);   // slam.cpp:434
        slam_agent.data_association(scan_measures, known_list);            // unknown_data_assoc.cpp:415
        mat lm = slam_agent.getStateLandmark();                             // slam.cpp:380
        (void)lm; (void)slam_agent.getStateX(); (void)slam_agent.getStateY(); (void)slam_agent.getStateTheta();
    }
};
// emitted, so that the object's undefined symbols are exactly the shim members a caller links against
void tick_once(Node& node, const rigid2d::Twist2D& tw) { node.tick(tw); }
int main() { return 0; }
