// MapPoint.h -- MOCK (test infrastructure) of the reference's MapPoint as far as the covisibility graph reads and writes it
// (Source/Libraries/ORB_SLAM2/include/MapPoint.h): same member names, everything public; and the member functions of the mock KeyFrame
// that need both classes.  They restate the reference's loops on the mocks' members and are the plain C++ reading the adapter
// csrc/host/Covisibility_hip.h is compared with.
#ifndef COVIS_MOCK_MAPPOINT_H
#define COVIS_MOCK_MAPPOINT_H
#include <stddef.h>

#include <algorithm>
#include <list>
#include <map>
#include <mutex>

#include "KeyFrame.h"

namespace ORB_SLAM2 {
class MapPoint {
 public:
  std::map<KeyFrame*, size_t> mObservations;
  int nObs = 0;
  bool mbBad = false;
  KeyFrame* mpRefKF = nullptr;
  std::mutex mMutexFeatures, mMutexPos;

  bool isBad() { std::unique_lock<std::mutex> lock(mMutexFeatures); std::unique_lock<std::mutex> lock2(mMutexPos); return mbBad; }
  std::map<KeyFrame*, size_t> GetObservations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mObservations; }
  int Observations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return nObs; }
  void AddObservation(KeyFrame* pKF, size_t idx) {
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs += pKF->mvuRight[idx] >= 0 ? 2 : 1;
  }
  void SetBadFlag() {
    std::map<KeyFrame*, size_t> obs;
    {
      std::unique_lock<std::mutex> lock1(mMutexFeatures);
      std::unique_lock<std::mutex> lock2(mMutexPos);
      mbBad = true;
      obs.swap(mObservations);
    }
    for (std::map<KeyFrame*, size_t>::iterator mit = obs.begin(); mit != obs.end(); ++mit) mit->first->EraseMapPointMatch(mit->second);
  }
  void EraseObservation(KeyFrame* pKF) {
    bool bBad = false;
    {
      std::unique_lock<std::mutex> lock(mMutexFeatures);
      std::map<KeyFrame*, size_t>::iterator it = mObservations.find(pKF);
      if (it != mObservations.end()) {
        nObs -= pKF->mvuRight[it->second] >= 0 ? 2 : 1;
        mObservations.erase(it);
        if (mpRefKF == pKF) mpRefKF = mObservations.empty() ? nullptr : mObservations.begin()->first;
        bBad = nObs <= 2;
      }
    }
    if (bBad) SetBadFlag();
  }
};

// the ordered vectors from the weights: ascending sort on (weight, pointer), then each pushed to the front
inline void KeyFrame::UpdateBestCovisibles() {
  std::unique_lock<std::mutex> lock(mMutexConnections);
  std::vector<std::pair<int, KeyFrame*> > vPairs;
  for (std::map<KeyFrame*, int>::iterator mit = mConnectedKeyFrameWeights.begin(); mit != mConnectedKeyFrameWeights.end(); ++mit)
    vPairs.push_back(std::make_pair(mit->second, mit->first));
  std::sort(vPairs.begin(), vPairs.end());
  std::list<KeyFrame*> lKFs;
  std::list<int> lWs;
  for (size_t i = 0; i < vPairs.size(); i++) {
    lKFs.push_front(vPairs[i].second);
    lWs.push_front(vPairs[i].first);
  }
  mvpOrderedConnectedKeyFrames.assign(lKFs.begin(), lKFs.end());
  mvOrderedWeights.assign(lWs.begin(), lWs.end());
}

// KeyFrame.cc:268-354 on the mock's members
inline void KeyFrame::UpdateConnections() {
  std::map<KeyFrame*, int> KFcounter;
  const std::vector<MapPoint*> vpMP = GetMapPointMatches();
  for (size_t i = 0; i < vpMP.size(); i++) {
    MapPoint* pMP = vpMP[i];
    if (!pMP || pMP->isBad()) continue;
    const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
    for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit)
      if (mit->first->mnId != mnId) KFcounter[mit->first]++;
  }
  if (KFcounter.empty()) return;
  int nmax = 0;
  KeyFrame* pKFmax = nullptr;
  const int th = 15;
  std::vector<std::pair<int, KeyFrame*> > vPairs;
  for (std::map<KeyFrame*, int>::iterator mit = KFcounter.begin(); mit != KFcounter.end(); ++mit) {
    if (mit->second > nmax) {
      nmax = mit->second;
      pKFmax = mit->first;
    }
    if (mit->second >= th) {
      vPairs.push_back(std::make_pair(mit->second, mit->first));
      mit->first->AddConnection(this, mit->second);
    }
  }
  if (vPairs.empty()) {
    vPairs.push_back(std::make_pair(nmax, pKFmax));
    pKFmax->AddConnection(this, nmax);
  }
  std::sort(vPairs.begin(), vPairs.end());
  std::list<KeyFrame*> lKFs;
  std::list<int> lWs;
  for (size_t i = 0; i < vPairs.size(); i++) {
    lKFs.push_front(vPairs[i].second);
    lWs.push_front(vPairs[i].first);
  }
  std::unique_lock<std::mutex> lock(mMutexConnections);
  mConnectedKeyFrameWeights = KFcounter;
  mvpOrderedConnectedKeyFrames.assign(lKFs.begin(), lKFs.end());
  mvOrderedWeights.assign(lWs.begin(), lWs.end());
  if (mbFirstConnection && mnId != 0) {
    mpParent = mvpOrderedConnectedKeyFrames.front();
    mpParent->AddChild(this);
    mbFirstConnection = false;
  }
}

// KeyFrame.cc:416-505 on the mock's members; a keyframe without a parent (the reference has none such) keeps its children
inline void KeyFrame::SetBadFlag() {
  {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    if (mnId == 0) return;
    if (mbNotErase) {
      mbToBeErased = true;
      return;
    }
  }
  for (std::map<KeyFrame*, int>::iterator mit = mConnectedKeyFrameWeights.begin(); mit != mConnectedKeyFrameWeights.end(); ++mit)
    mit->first->EraseConnection(this);
  for (size_t i = 0; i < mvpMapPoints.size(); i++)
    if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
  std::unique_lock<std::mutex> lock(mMutexConnections);
  std::unique_lock<std::mutex> lock1(mMutexFeatures);
  mConnectedKeyFrameWeights.clear();
  mvpOrderedConnectedKeyFrames.clear();
  std::set<KeyFrame*> sParentCandidates;
  if (mpParent) sParentCandidates.insert(mpParent);
  while (!mspChildrens.empty() && mpParent) {
    int max = -1;
    KeyFrame *pC = nullptr, *pP = nullptr;
    for (std::set<KeyFrame*>::iterator sit = mspChildrens.begin(); sit != mspChildrens.end(); ++sit) {
      KeyFrame* pKF = *sit;
      if (pKF->isBad()) continue;
      const std::vector<KeyFrame*> vpConnected = pKF->GetVectorCovisibleKeyFrames();
      for (size_t i = 0; i < vpConnected.size(); i++)
        for (std::set<KeyFrame*>::iterator spcit = sParentCandidates.begin(); spcit != sParentCandidates.end(); ++spcit)
          if (vpConnected[i]->mnId == (*spcit)->mnId) {
            const int w = pKF->GetWeight(vpConnected[i]);
            if (w > max) {
              pC = pKF;
              pP = vpConnected[i];
              max = w;
            }
          }
    }
    if (!pC) break;
    pC->ChangeParent(pP);
    sParentCandidates.insert(pC);
    mspChildrens.erase(pC);
  }
  if (mpParent) {
    for (std::set<KeyFrame*>::iterator sit = mspChildrens.begin(); sit != mspChildrens.end(); ++sit) (*sit)->ChangeParent(mpParent);
    mpParent->EraseChild(this);
  }
  mbBad = true;
}
}  // namespace ORB_SLAM2
#endif
